// kernels.hip -- CDNA4 (gfx950) kernels for the JPEG 2000 hot path.
//
//   * pointwise: DC level shift + RCT/ICT (forward), inverse RCT/ICT + DC
//     shift + clamp (TileProcessor.cpp:1449-1518 / 1303-1432, mct/mct.cpp)
//   * DWT: see dwt.hip
//   * T1: EBCOT encode / decode, one lane per code-block (t1_lane.h).
//   * gather: compacts per-code-block MQ output into one contiguous buffer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "grk_device.h"
#include "t1_flat.h"
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

namespace grkgpu {

__constant__ uint32_t c_mq_tab[47] = GRK_MQ_TABLE_INIT;

// ---------------------------------------------------------------------------
// pointwise
// ---------------------------------------------------------------------------
__device__ __forceinline__ int32_t fix_mul13(int32_t a, int32_t b) {
    int64_t t = (int64_t)a * (int64_t)b + 4096;
    return (int32_t)(t >> 13);
}

// NT: non-temporal stores (the output is streamed to HBM instead of lingering
// dirty in the caches for the next kernel to evict).
template <bool NT>
__device__ __forceinline__ void put(int32_t *p, int32_t v) {
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// one sample of type S at byte address p (any alignment); BE: stored
// most-significant byte first
template <typename S, bool BE>
__device__ __forceinline__ int32_t ld_sample(const uint8_t *p) {
    S v;
    __builtin_memcpy(&v, p, sizeof(S));
    if constexpr (BE) {
        static_assert(sizeof(S) == 2, "big-endian: 16-bit samples");
        v = (S)__builtin_bswap16((uint16_t)v);
    }
    return (int32_t)v;
}

// src: image planes of samples S (row stride sstride), dst: tile-component
// buffers (row stride tw).  One thread per sample of the tile.
template <bool NT, typename S>
__global__ void k_dcshift_mct_fwd(SrcPlanes src, uint32_t sstride, PlanePtrs dst, uint32_t tw, uint32_t th,
                                  uint32_t ncomp, ShiftArr shift, int32_t mct, int32_t irrev) {
    uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t y = blockIdx.y;
    if (x >= tw || y >= th) return;
    size_t si = (size_t)y * sstride + x, di = (size_t)y * tw + x;
    auto smp = [&](uint32_t c) { return (int32_t)((const S *)src.p[c])[si]; };
    uint32_t c0 = 0;
    if (mct && ncomp >= 3) {
        int32_t r = smp(0) - shift.v[0], g = smp(1) - shift.v[1], b = smp(2) - shift.v[2];
        int32_t o0, o1, o2;
        if (!irrev) {
            o0 = (r + (g * 2) + b) >> 2;
            o1 = b - g;
            o2 = r - g;
        } else {
            o0 = ict_term(r, 2449) + ict_term(g, 4809) + ict_term(b, 934);
            o1 = -ict_term(r, 1382) - ict_term(g, 2714) + ict_term(b, 4096);
            o2 = ict_term(r, 4096) - ict_term(g, 3430) - ict_term(b, 666);
        }
        put<NT>(&dst.p[0][di], o0); put<NT>(&dst.p[1][di], o1); put<NT>(&dst.p[2][di], o2);
        c0 = 3;
    }
    for (uint32_t c = c0; c < ncomp; ++c) {
        int32_t v = smp(c) - shift.v[c];
        put<NT>(&dst.p[c][di], irrev ? (int32_t)((uint32_t)v << 11) : v);
    }
}

// DC shift + custom array-based MCT (Part 2): TileProcessor.cpp:1449-1471
// then mct::encode_custom (mct.cpp:429-475) -- (x - shift) << 11, then per
// output component j the int32 sum over k of int_fix_mul(C[j][k], x_k), C the
// encoding matrix in 13-bit fixed point, in the reference's order.
// M: 0 = planar samples in host byte order; bit 0 = big-endian, bit 1 =
// interleaved (k_dcshift_mct_fwd_from's loads, any byte alignment).
template <typename S, int M = 0>
__global__ void k_dcshift_mct_custom(SrcPlanes src, uint32_t sstride, PlanePtrs dst, uint32_t tw, uint32_t th,
                                     uint32_t ncomp, ShiftArr shift, MctMatrix m) {
    uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t y = blockIdx.y;
    if (x >= tw || y >= th) return;
    size_t si = (size_t)y * sstride + x, di = (size_t)y * tw + x;
    auto smp = [&](uint32_t c) {
        if constexpr (M == 0) {
            return (int32_t)((const S *)src.p[c])[si];
        } else {
            const size_t srow = (size_t)y * sstride;
            const uint8_t *p = (M & 2) ? (const uint8_t *)src.p[0] + (srow + (size_t)x * ncomp + c) * sizeof(S)
                                       : (const uint8_t *)src.p[c] + (srow + x) * sizeof(S);
            return ld_sample<S, (M & 1) != 0>(p);
        }
    };
    int32_t v[GRK_MAX_COMPS];
    for (uint32_t c = 0; c < ncomp; ++c)
        v[c] = (int32_t)((uint32_t)(smp(c) - shift.v[c]) << 11);
    for (uint32_t j = 0; j < ncomp; ++j) {
        uint32_t acc = 0;
        for (uint32_t k = 0; k < ncomp; ++k)
            acc += (uint32_t)(int32_t)(((int64_t)m.c[j * ncomp + k] * (int64_t)v[k] + 4096) >> 13);
        put<true>(&dst.p[j][di], (int32_t)acc);
    }
}

// Inverse MCT + DC shift + clamp, tile buffers -> image planes.
__global__ void k_mct_inv_dcshift(PlanePtrs src, uint32_t sstride, uint32_t tw, uint32_t th, PlanePtrs dst,
                                  uint32_t dstride, uint32_t ncomp, ShiftArr shift, ShiftArr minv, ShiftArr maxv,
                                  int32_t mct, int32_t irrev) {
    uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t y = blockIdx.y;
    if (x >= tw || y >= th) return;
    size_t si = (size_t)y * sstride + x, di = (size_t)y * dstride + x;
    uint32_t c0 = 0;
    if (mct && ncomp >= 3) {
        int32_t o[3];
        if (!(irrev & 1)) {
            int32_t yv = src.p[0][si], u = src.p[1][si], v = src.p[2][si];
            int32_t g = yv - ((u + v) >> 2);
            o[0] = v + g; o[1] = g; o[2] = u + g;
        } else {
            float yv = __int_as_float(src.p[0][si]), u = __int_as_float(src.p[1][si]), v = __int_as_float(src.p[2][si]);
            // mct::decode_irrev (mct.cpp:352-408): separate mul/add, no FMA
            float r = __fadd_rn(yv, __fmul_rn(v, 1.402f));
            float g = __fsub_rn(__fsub_rn(yv, __fmul_rn(u, 0.34413f)), __fmul_rn(v, 0.71414f));
            float b = __fadd_rn(yv, __fmul_rn(u, 1.772f));
            o[0] = (int32_t)rintf(r); o[1] = (int32_t)rintf(g); o[2] = (int32_t)rintf(b);
        }
        for (int c = 0; c < 3; ++c) {
            int32_t v = o[c] + shift.v[c];
            dst.p[c][di] = v < minv.v[c] ? minv.v[c] : (v > maxv.v[c] ? maxv.v[c] : v);
        }
        c0 = 3;
    }
    for (uint32_t c = c0; c < ncomp; ++c) {
        int32_t v = src.p[c][si];
        if ((irrev >> c) & 1) v = (int32_t)rintf(__int_as_float(v));
        v += shift.v[c];
        dst.p[c][di] = v < minv.v[c] ? minv.v[c] : (v > maxv.v[c] ? maxv.v[c] : v);
    }
}

// Inverse MCT + DC shift + clamp straight to the caller's sample type T
// (uint8 / int8 / uint16 / int16, or int32 for the interleaved layout) and
// layout -- k_mct_inv_dcshift's arithmetic, statement for statement; only the
// store differs.  The clamp to the component's [min, max] comes first and the
// format holds that range (checked by the callers), so the narrowing is exact.
//
// A thread owns a run of RUN = 16 / sizeof(T) adjacent pixels of one row: it
// reads each component's coefficients as dwordx4 where the source is 16-byte
// aligned and writes the run as packed words -- one dwordx4 per component
// (planar), ncomp dwordx4 (interleaved, 16 * ncomp bytes).  Runs are laid on
// the destination's 16-byte grid: thread 0 of a row takes the `lead` pixels
// before the first aligned address (scalar stores), thread t > 0 the run from
// lead + (t - 1) * RUN, and the row's last run is cut at tw (scalar stores).
// Where a full run's address still is not 16-byte aligned (another plane's
// base, a row pitch that moves it) it goes out as dwords if 4-byte aligned
// and as single samples otherwise: every byte offset is correct, the aligned
// interior is fast.  Stores are non-temporal: nothing on the device reads the
// image again.
template <typename T>
struct NarrowRun { static constexpr int N = 16 / (int)sizeof(T); };

// Float destinations (SMP_F32 / _F16 / _BF16, the float decode entry points
// only): tag types of the destination's sample size, so that everything sized
// by sizeof(T) -- the run length, run_of, the row threads -- works as for the
// integer formats.  A float store always has OutOps (OP != 0): behind the
// precision op, norm_run replaces a run's finished int32 values by the bit
// patterns of their float32 images v * scale + bias; pack_word / store_sample
// then round those to the destination's format, to nearest even (gfx950:
// v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32; denormals are kept, overflow is inf).
struct SmpF32 { uint32_t bits; };
struct SmpF16 { uint16_t bits; };
struct SmpBF16 { uint16_t bits; };
template <typename T>
constexpr bool float_tag = std::is_same<T, SmpF32>::value || std::is_same<T, SmpF16>::value || std::is_same<T, SmpBF16>::value;

// channel ch's values -> float32 bit patterns: the product and the sum each
// rounded on their own (no FMA, as in inv_mct_run); nothing for an integer T
template <typename T, int N>
__device__ __forceinline__ void norm_run([[maybe_unused]] int32_t (&v)[N], [[maybe_unused]] const OutOps &o,
                                         [[maybe_unused]] uint32_t ch) {
    if constexpr (float_tag<T>) {
#pragma clang fp contract(off)
        const float s = o.scale[ch], b = o.bias[ch];
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = __float_as_int(__fadd_rn(__fmul_rn((float)v[i], s), b));
    }
}
// Two float32 bit patterns as one word of two 16-bit floats, low address
// first: gfx950's packed conversions, which round to nearest even under the
// kernels' mode (what the compiler selects for a <2 x float> truncation).
// Spelled as the instruction: written as a vector conversion of two adjacent
// elements of a run, the run's array is promoted to one 32-wide vector value
// that is copied at every element write -- k_mct_inv_dcshift_pixels<SmpF16, 4,
// OP_PREC> then takes 128 VGPRs and 1320 bytes of scratch where its uint16 form
// takes 45 VGPRs and none.
template <typename T>
__device__ __forceinline__ uint32_t pack_floats(int32_t a, int32_t b) {
    uint32_t r;
    if constexpr (std::is_same<T, SmpF16>::value)
        asm("v_cvt_pk_f16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    else
        asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// one finished value to its sample at p (a float T: v is norm_run's bit pattern)
template <typename T>
__device__ __forceinline__ void store_sample(int32_t v, T *p) {
    if constexpr (std::is_same<T, SmpF32>::value)
        __builtin_nontemporal_store((uint32_t)v, (uint32_t *)p);
    else if constexpr (std::is_same<T, SmpF16>::value)
        __builtin_nontemporal_store(__builtin_bit_cast(uint16_t, (_Float16)__int_as_float(v)), (uint16_t *)p);
    else if constexpr (std::is_same<T, SmpBF16>::value)
        __builtin_nontemporal_store(__builtin_bit_cast(uint16_t, (__bf16)__int_as_float(v)), (uint16_t *)p);
    else
        __builtin_nontemporal_store((T)v, p);
}

// one word of a run: samples [j * 4 / sizeof(T), ...) of v, low address first
template <typename T>
__device__ __forceinline__ uint32_t pack_word(const int32_t *v, int j) {
    if constexpr (float_tag<T> && sizeof(T) == 2)
        return pack_floats<T>(v[2 * j], v[2 * j + 1]);
    else if constexpr (sizeof(T) == 1)
        return ((uint32_t)v[4 * j] & 0xffu) | (((uint32_t)v[4 * j + 1] & 0xffu) << 8) |
               (((uint32_t)v[4 * j + 2] & 0xffu) << 16) | ((uint32_t)v[4 * j + 3] << 24);
    else if constexpr (sizeof(T) == 2)
        return ((uint32_t)v[2 * j] & 0xffffu) | ((uint32_t)v[2 * j + 1] << 16);
    else
        return (uint32_t)v[j];
}

// NS samples (a multiple of a 16-byte group; static indices only, so v stays
// in registers), of which the first n are stored
template <typename T, int NS>
__device__ __forceinline__ void store_samples(T *p, const int32_t (&v)[NS], int n) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr int G = NarrowRun<T>::N;  // samples per 16 bytes
    const uintptr_t a = (uintptr_t)p;
    if (n == NS && !(a & 15)) {
#pragma unroll
        for (int g = 0; g < NS / G; ++g) {
            const u32x4 w = {pack_word<T>(v + g * G, 0), pack_word<T>(v + g * G, 1), pack_word<T>(v + g * G, 2),
                             pack_word<T>(v + g * G, 3)};
            __builtin_nontemporal_store(w, (u32x4 *)p + g);
        }
    } else if (n == NS && !(a & 3)) {
#pragma unroll
        for (int j = 0; j < NS / G * 4; ++j)
            __builtin_nontemporal_store(pack_word<T>(v + (j / 4) * G, j % 4), (uint32_t *)p + j);
    } else {
#pragma unroll
        for (int i = 0; i < NS; ++i)
            if (i < n) store_sample<T>(v[i], p + i);
    }
}

// n <= N coefficients of one component's row
template <int N>
__device__ __forceinline__ void load_run(const int32_t *p, int n, int32_t (&v)[N]) {
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    if (n == N && !((uintptr_t)p & 15)) {
#pragma unroll
        for (int g = 0; g < N / 4; ++g) {
            const i32x4 q = ((const i32x4 *)p)[g];
            v[4 * g] = q.x; v[4 * g + 1] = q.y; v[4 * g + 2] = q.z; v[4 * g + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = i < n ? p[i] : 0;
    }
}

// the run of thread t of a row whose first sample lies at byte address a and
// whose pixels are pxb bytes: first pixel and pixel count (0: none)
template <int N>
__device__ __forceinline__ int run_of(uintptr_t a, uint32_t pxb, uint32_t t, uint32_t tw, uint32_t &x0) {
    uint32_t lead = 0;  // pixels before the first 16-byte boundary a run can start on (none: runs from 0)
    for (uint32_t l = 0; l < (uint32_t)N; ++l)
        if (!((a + (uintptr_t)l * pxb) & 15)) { lead = l; break; }
    const uint64_t first = t ? (uint64_t)lead + (uint64_t)(t - 1) * N : 0;
    const uint64_t end = t ? first + N : lead;
    x0 = (uint32_t)(first < tw ? first : tw);
    return (int)((end < tw ? end : tw) - x0);
}

// the three MCT components of n pixels: k_mct_inv_dcshift's first branch
template <int N>
__device__ __forceinline__ void inv_mct_run(int32_t (&a)[N], int32_t (&b)[N], int32_t (&c)[N], int32_t irrev,
                                            const ShiftArr &shift, const ShiftArr &minv, const ShiftArr &maxv) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        int32_t o[3];
        if (!(irrev & 1)) {
            int32_t yv = a[i], u = b[i], v = c[i];
            int32_t g = yv - ((u + v) >> 2);
            o[0] = v + g; o[1] = g; o[2] = u + g;
        } else {
            float yv = __int_as_float(a[i]), u = __int_as_float(b[i]), v = __int_as_float(c[i]);
            // mct::decode_irrev (mct.cpp:352-408): separate mul/add, no FMA
            float r = __fadd_rn(yv, __fmul_rn(v, 1.402f));
            float g = __fsub_rn(__fsub_rn(yv, __fmul_rn(u, 0.34413f)), __fmul_rn(v, 0.71414f));
            float bl = __fadd_rn(yv, __fmul_rn(u, 1.772f));
            o[0] = (int32_t)rintf(r); o[1] = (int32_t)rintf(g); o[2] = (int32_t)rintf(bl);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            int32_t v = o[k] + shift.v[k];
            o[k] = v < minv.v[k] ? minv.v[k] : (v > maxv.v[k] ? maxv.v[k] : v);
        }
        a[i] = o[0]; b[i] = o[1]; c[i] = o[2];
    }
}

// a component outside the MCT: k_mct_inv_dcshift's second loop
template <int N>
__device__ __forceinline__ void inv_plain_run(int32_t (&a)[N], int32_t irrev_c, int32_t shift, int32_t mn, int32_t mx) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        int32_t v = a[i];
        if (irrev_c) v = (int32_t)rintf(__int_as_float(v));
        v += shift;
        a[i] = v < mn ? mn : (v > mx ? mx : v);
    }
}

// ---------------------------------------------------------------------------
// The output conversions (OutOps, grk_device.h) on a run's finished values,
// between the clamp / replication and store_samples.  The kernels below carry
// them as the template parameter OP: 0 = none (the instantiations every decode
// without ops runs: no ops argument, the code as it was), OP_PREC = the
// precision op of each component, OP_SYCC = sYCC -> RGB on the three
// components, then their precision ops; OP_EYCC = eYCC -> RGB in their place;
// OP_CMYK = CMYK -> RGB on components 0 .. 3, which leaves one channel fewer
// than there are components (OutOps: COL_EYCC / COL_CMYK).
// ---------------------------------------------------------------------------
constexpr int OP_PREC = 1, OP_SYCC = 2, OP_EYCC = 3, OP_CMYK = 4;
// a conversion of exactly three components, with or without an MCT
constexpr bool op_ycc(int op) { return op == OP_SYCC || op == OP_EYCC; }
// the component output channel c carries: c, or behind CMYK's black ink c + 1
constexpr int chan_comp(int op, int c) { return op == OP_CMYK && c >= 3 ? c + 1 : c; }

// clip_component / scale_component (convert.cpp:82-161); o is uniform over the
// launch, so the switch does not diverge
template <int N>
__device__ __forceinline__ void prec_run(int32_t (&v)[N], const PrecOp &o) {
    const int32_t a = o.a, b = o.b;
    switch (o.mode) {
        case POP_CLIP:
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = v[i] < a ? a : (v[i] > b ? b : v[i]);
            break;
        case POP_SHR:
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] >>= a;
            break;
        case POP_MULDIV:  // plain 32-bit division: exact
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = (int32_t)((uint32_t)v[i] * (uint32_t)a / (uint32_t)b);
            break;
        case POP_MUL:
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] *= a;
            break;
        default: break;
    }
}

// sycc_to_rgb (color.cpp:136-162): the three terms depend on the chroma pair
// only -- (int32_t)(1.402 * cr), (int32_t)(0.344 * cb + 0.714 * cr),
// (int32_t)(1.772 * cb) in IEEE double, every product and the sum rounded on
// its own (no FMA), the conversion truncating
// __dmul_rn / __dadd_rn are plain * and + to the compiler: what keeps them
// apart is that nothing here may be contracted, whatever flags the file is
// built with -- hence the pragma, not only the Makefile's -ffp-contract=off.
__device__ __forceinline__ void sycc_terms(int32_t cb, int32_t cr, int32_t off, int32_t &tr, int32_t &tg,
                                           int32_t &tb) {
#pragma clang fp contract(off)
    const double b = (double)(cb - off), r = (double)(cr - off);
    tr = (int32_t)__dmul_rn(1.402, r);
    tg = (int32_t)__dadd_rn(__dmul_rn(0.344, b), __dmul_rn(0.714, r));
    tb = (int32_t)__dmul_rn(1.772, b);
}
__device__ __forceinline__ int32_t clamp_upb(int32_t v, int32_t upb) { return v < 0 ? 0 : (v > upb ? upb : v); }
// ... and the pixel: y, the chroma terms -> R, G, B
__device__ __forceinline__ void sycc_pixel(int32_t y, int32_t tr, int32_t tg, int32_t tb, int32_t upb, int32_t &r,
                                           int32_t &g, int32_t &b) {
    r = clamp_upb(y + tr, upb);
    g = clamp_upb(y - tg, upb);
    b = clamp_upb(y + tb, upb);
}
// N pixels with a chroma pair each (4:4:4)
template <int N>
__device__ __forceinline__ void sycc_run(int32_t (&a)[N], int32_t (&b)[N], int32_t (&c)[N], const OutOps &ops) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        int32_t tr, tg, tb;
        sycc_terms(b[i], c[i], ops.off, tr, tg, tb);
        sycc_pixel(a[i], tr, tg, tb, ops.upb, a[i], b[i], c[i]);
    }
}

// color_esycc_to_rgb (color.cpp:936-995): IEEE double, the source line's
// operations one by one from the left, each rounded on its own (no
// contraction, as in sycc_terms), the conversion truncating
__device__ __forceinline__ void eycc_pixel(int32_t &y, int32_t &u, int32_t &v, const OutOps &ops) {
#pragma clang fp contract(off)
    const double yv = (double)y, cb = (double)(u - ops.coff[0]), cr = (double)(v - ops.coff[1]);
    const int32_t r = (int32_t)(yv - 0.0000368 * cb + 1.40199 * cr + 0.5);
    const int32_t g = (int32_t)(1.0003 * yv - 0.344125 * cb - 0.7141128 * cr + 0.5);
    const int32_t b = (int32_t)(0.999823 * yv + 1.77204 * cb - 0.000008 * cr + 0.5);
    y = clamp_upb(r, ops.upb);
    u = clamp_upb(g, ops.upb);
    v = clamp_upb(b, ops.upb);
}
template <int N>
__device__ __forceinline__ void eycc_run(int32_t (&a)[N], int32_t (&b)[N], int32_t (&c)[N], const OutOps &ops) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
        eycc_pixel(a[i], b[i], c[i], ops);
        // One pixel's doubles at a time: left to itself the compiler converts a 16-pixel run to doubles
        // first and spills (800 scratch instructions).  The empty statement makes the next pixel's inputs
        // depend on this pixel's results, which is an order instruction selection has to keep.
        if constexpr (N > 4) {
            if (i + 1 < N)
                asm volatile("" : "+v"(a[i]), "+v"(b[i]), "+v"(c[i]), "+v"(a[i + 1]), "+v"(b[i + 1]), "+v"(c[i + 1]));
        }
    }
}
// the conversion of a three-component OP
template <int OP, int N>
__device__ __forceinline__ void ycc_run(int32_t (&a)[N], int32_t (&b)[N], int32_t (&c)[N], const OutOps &ops) {
    if constexpr (OP == OP_SYCC) sycc_run<N>(a, b, c, ops);
    else eycc_run<N>(a, b, c, ops);
}

// color_cmyk_to_rgb (color.cpp:881-933): float32, every operation rounded on
// its own, the conversion truncating; the scales come divided from the host.
// In-range unsigned inks give 0 .. 255, so nothing is clamped.
__device__ __forceinline__ void cmyk_pixel(int32_t &c, int32_t &m, int32_t &y, int32_t k, const OutOps &ops) {
#pragma clang fp contract(off)
    const float C = 1.0f - (float)c * ops.sc[0], M = 1.0f - (float)m * ops.sc[1];
    const float Y = 1.0f - (float)y * ops.sc[2], K = 1.0f - (float)k * ops.sc[3];
    c = (int32_t)(255.0f * C * K);
    m = (int32_t)(255.0f * M * K);
    y = (int32_t)(255.0f * Y * K);
}
template <int N>
__device__ __forceinline__ void cmyk_run(int32_t (&a)[N], int32_t (&b)[N], int32_t (&c)[N], const int32_t (&k)[N],
                                         const OutOps &ops) {
#pragma unroll
    for (int i = 0; i < N; ++i) cmyk_pixel(a[i], b[i], c[i], k[i], ops);
}

// The kernels take the ops as a trailing parameter pack O: empty for OP = 0, so
// those instantiations keep the parameters and the code they always had, and
// one OutOps otherwise.
__device__ __forceinline__ const OutOps *ops_ptr() { return nullptr; }
__device__ __forceinline__ const OutOps *ops_ptr(const OutOps &o) { return &o; }

template <typename T>
__device__ __forceinline__ void store_packed(T *p, const uint32_t (&w)[4], int n);  // (below)
// 4 samples packed behind the ones a run's 16 bytes already hold (k_mct_inv_custom_planar's push)
template <typename T>
__device__ __forceinline__ void push_packed(uint32_t (&p)[4], const int32_t (&v)[4]) {
    constexpr int W = (int)sizeof(T);
#pragma unroll
    for (int w = 0; w + W < 4; ++w) p[w] = p[w + W];
#pragma unroll
    for (int w = 0; w < W; ++w) p[4 - W + w] = pack_word<T>(v, w);
}

// OP_CMYK, planar: the run's R, G, B planes from its four ink planes, walked
// in sub-runs of 4 pixels as k_mct_inv_custom_planar walks its run, so that an
// 8-bit run never holds its 4 x 16 inks as floats at once
template <typename T>
__device__ __forceinline__ void cmyk_planar_run(const PlanePtrs &src, size_t si, const DstPlanes &dst, size_t di, int n,
                                                const ShiftArr &shift, const ShiftArr &minv, const ShiftArr &maxv,
                                                int32_t mct, int32_t irrev, const OutOps &ops) {
    constexpr int N = NarrowRun<T>::N;
    uint32_t pk[3][4];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int w = 0; w < 4; ++w) pk[j][w] = 0;
#pragma unroll 1
    for (int s = 0; s < N / 4; ++s) {
        const int left = n - 4 * s, ms = left < 0 ? 0 : (left > 4 ? 4 : left);
        int32_t v[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k) load_run<4>(src.p[k] + si + 4 * s, ms, v[k]);
        if (mct) inv_mct_run<4>(v[0], v[1], v[2], irrev, shift, minv, maxv);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (!mct || k == 3) inv_plain_run<4>(v[k], (irrev >> k) & 1, shift.v[k], minv.v[k], maxv.v[k]);
        cmyk_run<4>(v[0], v[1], v[2], v[3], ops);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            prec_run<4>(v[j], ops.pc[j]);
            norm_run<T, 4>(v[j], ops, j);
            push_packed<T>(pk[j], v[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) store_packed<T>((T *)dst.p[j] + di, pk[j], n);
}

// The three bodies of that store, shared by the per-tile kernels below (the
// pixel run excepted) and the job-table kernel k_store_jobs: thread t of row y finishes its run and
// stores it.  Every argument is uniform over the workgroup.  KMAX is the
// component count the caller's src / dst hold: GRK_MAX_COMPS for kernel
// arguments, which the loops index at run time, or 4 for a StoreJob's, which
// sit in scalar registers and so take static indices only (the loops unrolled
// behind uniform guards).  ops: null exactly when OP = 0.
//
// component k outside the MCT and the colour conversion: its n samples at si,
// finished, through the precision op of channel ch, to that channel's plane
// at di (each address is formed where it is used, not before)
template <typename T, int OP>
__device__ __forceinline__ void store_plain_run(const PlanePtrs &src, size_t si, const DstPlanes &dst, size_t di, int n,
                                                uint32_t k, uint32_t ch, int32_t irrev, const ShiftArr &shift,
                                                const ShiftArr &minv, const ShiftArr &maxv,
                                                [[maybe_unused]] const OutOps *ops) {
    constexpr int N = NarrowRun<T>::N;
    int32_t a[N];
    load_run<N>(src.p[k] + si, n, a);
    inv_plain_run<N>(a, (irrev >> k) & 1, shift.v[k], minv.v[k], maxv.v[k]);
    if constexpr (OP != 0) {
        prec_run<N>(a, ops->pc[ch]);
        norm_run<T, N>(a, *ops, ch);
    }
    store_samples<T, N>((T *)dst.p[ch] + di, a, n);
}

// planar: dst.p[c] = plane c (samples T), rows dstride samples apart
template <typename T, int OP, int KMAX = GRK_MAX_COMPS>
__device__ __forceinline__ void store_planar_run(const PlanePtrs &src, uint32_t sstride, uint32_t tw,
                                                 const DstPlanes &dst, uint32_t dstride, uint32_t ncomp, uint32_t y, uint32_t t,
                                                 const ShiftArr &shift, const ShiftArr &minv, const ShiftArr &maxv,
                                                 int32_t mct, int32_t irrev, [[maybe_unused]] const OutOps *ops) {
    constexpr int N = NarrowRun<T>::N;
    const size_t drow = (size_t)y * dstride;
    uint32_t x0;
    const int n = run_of<N>((uintptr_t)((T *)dst.p[0] + drow), sizeof(T), t, tw, x0);
    if (n <= 0) return;
    const size_t si = (size_t)y * sstride + x0, di = drow + x0;
    if constexpr (OP == OP_CMYK) {  // four or more components: channels R, G, B, then components 4 ..
        cmyk_planar_run<T>(src, si, dst, di, n, shift, minv, maxv, mct, irrev, *ops);
        if constexpr (KMAX > 4)
            for (uint32_t k = 4; k < ncomp; ++k)
                store_plain_run<T, OP>(src, si, dst, di, n, k, k - 1, irrev, shift, minv, maxv, ops);
        return;
    }
    // (sYCC / eYCC: exactly three components, with or without an MCT)
    const bool three = op_ycc(OP) || (mct && ncomp >= 3);
    uint32_t c0 = 0;
    if (three) {
        int32_t a[N], b[N], c[N];
        load_run<N>(src.p[0] + si, n, a);
        load_run<N>(src.p[1] + si, n, b);
        load_run<N>(src.p[2] + si, n, c);
        if (!op_ycc(OP) || mct) {
            inv_mct_run<N>(a, b, c, irrev, shift, minv, maxv);
        } else {
            inv_plain_run<N>(a, irrev & 1, shift.v[0], minv.v[0], maxv.v[0]);
            inv_plain_run<N>(b, (irrev >> 1) & 1, shift.v[1], minv.v[1], maxv.v[1]);
            inv_plain_run<N>(c, (irrev >> 2) & 1, shift.v[2], minv.v[2], maxv.v[2]);
        }
        if constexpr (op_ycc(OP)) ycc_run<OP, N>(a, b, c, *ops);
        if constexpr (OP != 0) {
            prec_run<N>(a, ops->pc[0]);
            prec_run<N>(b, ops->pc[1]);
            prec_run<N>(c, ops->pc[2]);
            norm_run<T, N>(a, *ops, 0);
            norm_run<T, N>(b, *ops, 1);
            norm_run<T, N>(c, *ops, 2);
        }
        store_samples<T, N>((T *)dst.p[0] + di, a, n);
        store_samples<T, N>((T *)dst.p[1] + di, b, n);
        store_samples<T, N>((T *)dst.p[2] + di, c, n);
        c0 = 3;
    }
    if constexpr (KMAX > 4) {
        // store_plain_run's statements, in place: a call from this loop costs the 8-bit
        // precision-op kernels a wave per SIMD (74 VGPRs for 71 in the compiler's report)
        for (uint32_t k = c0; k < ncomp; ++k) {
            int32_t a[N];
            load_run<N>(src.p[k] + si, n, a);
            inv_plain_run<N>(a, (irrev >> k) & 1, shift.v[k], minv.v[k], maxv.v[k]);
            if constexpr (OP != 0) {
                prec_run<N>(a, ops->pc[k]);
                norm_run<T, N>(a, *ops, k);
            }
            store_samples<T, N>((T *)dst.p[k] + di, a, n);
        }
    } else {
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if ((uint32_t)k < ncomp && !(three && k < 3))
                store_plain_run<T, OP>(src, si, dst, di, n, k, k, irrev, shift, minv, maxv, ops);
    }
}

// interleaved, NC = 3 or 4 components (OP_CMYK: 4 or 5, one channel fewer):
// sample (y, x, c) at dst0[y * dstride + x * NCH + c].  The job-table kernel's
// form of k_mct_inv_dcshift_pixels' body below, which has to keep the
// statements in the kernel (see there).
template <typename T, int NC, int OP>
__device__ __forceinline__ void store_pixels_run(const PlanePtrs &src, uint32_t sstride, uint32_t tw, void *dst0,
                                                 uint32_t dstride, uint32_t y, uint32_t t, const ShiftArr &shift,
                                                 const ShiftArr &minv, const ShiftArr &maxv, int32_t mct, int32_t irrev,
                                                 [[maybe_unused]] const OutOps *ops) {
    static_assert(!op_ycc(OP) || NC == 3, "sYCC / eYCC: three components");
    static_assert(OP != OP_CMYK || NC >= 4, "CMYK: four inks");
    constexpr int N = NarrowRun<T>::N;
    // the pixels stored: NCH channels each (OP_CMYK: one fewer than the components read)
    constexpr int NCH = OP == OP_CMYK ? NC - 1 : NC;
    T *const drow = (T *)dst0 + (size_t)y * dstride;
    uint32_t x0;
    const int n = run_of<N>((uintptr_t)drow, NCH * sizeof(T), t, tw, x0);
    if (n <= 0) return;
    const size_t si = (size_t)y * sstride + x0;
    int32_t v[NC][N];
#pragma unroll
    for (int k = 0; k < NC; ++k) load_run<N>(src.p[k] + si, n, v[k]);
    if (mct) inv_mct_run<N>(v[0], v[1], v[2], irrev, shift, minv, maxv);
#pragma unroll
    for (int k = 0; k < NC; ++k)
        if (!mct || k >= 3) inv_plain_run<N>(v[k], (irrev >> k) & 1, shift.v[k], minv.v[k], maxv.v[k]);
    if constexpr (op_ycc(OP)) ycc_run<OP, N>(v[0], v[1], v[2], *ops);
    if constexpr (OP == OP_CMYK) cmyk_run<N>(v[0], v[1], v[2], v[3], *ops);
    if constexpr (OP != 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            prec_run<N>(v[chan_comp(OP, c)], ops->pc[c]);
            norm_run<T, N>(v[chan_comp(OP, c)], *ops, c);
        }
    }
    int32_t px[N * NCH];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int c = 0; c < NCH; ++c) px[i * NCH + c] = v[chan_comp(OP, c)][i];
    store_samples<T, N * NCH>(drow + (size_t)x0 * NCH, px, n * NCH);
}

// ... and one sample of such a component to its channel of the pixel at d (the thread-per-pixel form)
template <typename T, int OP>
__device__ __forceinline__ void store_plain_sample(const PlanePtrs &src, size_t si, T *d, uint32_t k, uint32_t ch,
                                                   int32_t irrev, const ShiftArr &shift, const ShiftArr &minv,
                                                   const ShiftArr &maxv, [[maybe_unused]] const OutOps *ops) {
    int32_t a[1] = {src.p[k][si]};
    inv_plain_run<1>(a, (irrev >> k) & 1, shift.v[k], minv.v[k], maxv.v[k]);
    if constexpr (OP != 0) {
        prec_run<1>(a, ops->pc[ch]);
        norm_run<T, 1>(a, *ops, ch);
    }
    store_sample<T>(a[0], d + ch);
}

// interleaved, any other component count: pixel x of row y, one store per
// sample
template <typename T, int OP, int KMAX = GRK_MAX_COMPS>
__device__ __forceinline__ void store_pixel_any(const PlanePtrs &src, uint32_t sstride, void *dst0, uint32_t dstride,
                                                uint32_t ncomp, uint32_t y, uint32_t x, const ShiftArr &shift,
                                                const ShiftArr &minv, const ShiftArr &maxv, int32_t mct, int32_t irrev,
                                                [[maybe_unused]] const OutOps *ops) {
    const size_t si = (size_t)y * sstride + x;
    if constexpr (OP == OP_CMYK) {  // ncomp >= 4 components, pixels of ncomp - 1 channels
        T *const d = (T *)dst0 + (size_t)y * dstride + (size_t)x * (ncomp - 1);
        int32_t v[4][1];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k][0] = src.p[k][si];
        if (mct) inv_mct_run<1>(v[0], v[1], v[2], irrev, shift, minv, maxv);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (!mct || k == 3) inv_plain_run<1>(v[k], (irrev >> k) & 1, shift.v[k], minv.v[k], maxv.v[k]);
        cmyk_run<1>(v[0], v[1], v[2], v[3], *ops);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            prec_run<1>(v[j], ops->pc[j]);
            norm_run<T, 1>(v[j], *ops, j);
            store_sample<T>(v[j][0], d + j);
        }
        if constexpr (KMAX > 4)
            for (uint32_t k = 4; k < ncomp; ++k)
                store_plain_sample<T, OP>(src, si, d, k, k - 1, irrev, shift, minv, maxv, ops);
        return;
    }
    T *const d = (T *)dst0 + (size_t)y * dstride + (size_t)x * ncomp;
    uint32_t c0 = 0;
    if (mct && ncomp >= 3) {
        int32_t a[1] = {src.p[0][si]}, b[1] = {src.p[1][si]}, c[1] = {src.p[2][si]};
        inv_mct_run<1>(a, b, c, irrev, shift, minv, maxv);
        if constexpr (OP != 0) {
            prec_run<1>(a, ops->pc[0]);
            prec_run<1>(b, ops->pc[1]);
            prec_run<1>(c, ops->pc[2]);
            norm_run<T, 1>(a, *ops, 0);
            norm_run<T, 1>(b, *ops, 1);
            norm_run<T, 1>(c, *ops, 2);
        }
        store_sample<T>(a[0], d);
        store_sample<T>(b[0], d + 1);
        store_sample<T>(c[0], d + 2);
        c0 = 3;
    }
    if constexpr (KMAX > 4) {
        for (uint32_t k = c0; k < ncomp; ++k)
            store_plain_sample<T, OP>(src, si, d, k, k, irrev, shift, minv, maxv, ops);
    } else {
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if ((uint32_t)k >= c0 && (uint32_t)k < ncomp)
                store_plain_sample<T, OP>(src, si, d, k, k, irrev, shift, minv, maxv, ops);
    }
}

// The per-tile kernels: a (row threads, rows) grid in front of those bodies.
template <typename T, int OP = 0, typename... O>
__global__ void k_mct_inv_dcshift_planar(PlanePtrs src, uint32_t sstride, uint32_t tw, uint32_t th, DstPlanes dst,
                                         uint32_t dstride, uint32_t ncomp, ShiftArr shift, ShiftArr minv,
                                         ShiftArr maxv, int32_t mct, int32_t irrev, O... o) {
    static_assert(sizeof...(O) == (OP != 0), "one OutOps exactly when OP != 0");
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (y >= th) return;
    store_planar_run<T, OP>(src, sstride, tw, dst, dstride, ncomp, y, t, shift, minv, maxv, mct, irrev, ops_ptr(o...));
}

template <typename T, int NC, int OP = 0, typename... O>
__global__ void k_mct_inv_dcshift_pixels(PlanePtrs src, uint32_t sstride, uint32_t tw, uint32_t th, DstPlanes dst,
                                         uint32_t dstride, ShiftArr shift, ShiftArr minv, ShiftArr maxv, int32_t mct,
                                         int32_t irrev, O... o) {
    static_assert(sizeof...(O) == (OP != 0), "one OutOps exactly when OP != 0");
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (y >= th) return;
    // store_pixels_run's statements, in place: behind a call the compiler fetches the plane pointers and
    // clamp arrays ahead of the branches that use them, and the 8-bit RGB store then takes 0.032 ms for
    // 0.028 on a 4K frame (MI355X, profiles/last_store_ab.json)
    [[maybe_unused]] const OutOps *const ops = ops_ptr(o...);
    constexpr int N = NarrowRun<T>::N;
    constexpr int NCH = OP == OP_CMYK ? NC - 1 : NC;
    T *const drow = (T *)dst.p[0] + (size_t)y * dstride;
    uint32_t x0;
    const int n = run_of<N>((uintptr_t)drow, NCH * sizeof(T), t, tw, x0);
    if (n <= 0) return;
    const size_t si = (size_t)y * sstride + x0;
    int32_t v[NC][N];
#pragma unroll
    for (int k = 0; k < NC; ++k) load_run<N>(src.p[k] + si, n, v[k]);
    if (mct) inv_mct_run<N>(v[0], v[1], v[2], irrev, shift, minv, maxv);
#pragma unroll
    for (int k = 0; k < NC; ++k)
        if (!mct || k >= 3) inv_plain_run<N>(v[k], (irrev >> k) & 1, shift.v[k], minv.v[k], maxv.v[k]);
    if constexpr (op_ycc(OP)) ycc_run<OP, N>(v[0], v[1], v[2], *ops);
    if constexpr (OP == OP_CMYK) cmyk_run<N>(v[0], v[1], v[2], v[3], *ops);
    if constexpr (OP != 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) {
            prec_run<N>(v[chan_comp(OP, c)], ops->pc[c]);
            norm_run<T, N>(v[chan_comp(OP, c)], *ops, c);
        }
    }
    int32_t px[N * NCH];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int c = 0; c < NCH; ++c) px[i * NCH + c] = v[chan_comp(OP, c)][i];
    store_samples<T, N * NCH>(drow + (size_t)x0 * NCH, px, n * NCH);
}

template <typename T, int OP = 0, typename... O>
__global__ void k_mct_inv_dcshift_pixels_any(PlanePtrs src, uint32_t sstride, uint32_t tw, uint32_t th, DstPlanes dst,
                                             uint32_t dstride, uint32_t ncomp, ShiftArr shift, ShiftArr minv,
                                             ShiftArr maxv, int32_t mct, int32_t irrev, O... o) {
    static_assert(sizeof...(O) == (OP != 0), "one OutOps exactly when OP != 0");
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= tw || y >= th) return;
    store_pixel_any<T, OP>(src, sstride, dst.p[0], dstride, ncomp, y, x, shift, minv, maxv, mct, irrev, ops_ptr(o...));
}

// ---------------------------------------------------------------------------
// Inverse custom (Part 2 array-based) MCT + offsets + clamp, tile buffers ->
// the caller's samples: mct::decode_custom (mct.cpp:477-511) followed by
// dc_level_shift_decode's irreversible branch (TileProcessor.cpp:1377-1432),
// statement for statement.  Per pixel and output component j
//     acc = 0.0f;  for k ascending: acc = acc + D[j][k] * x_k
//     out_j = clamp((int32) lrintf(acc) + off_j, min_j, max_j)
// every product and sum rounded on its own in float32 (no FMA), which is why
// this is VALU work and not an MFMA: the matrix cores sum in another order.
// The inverse of k_dcshift_mct_custom.  Matrix, offsets and clamp bounds are
// uniform over the launch and arrive by value (scalar loads).
//
// Run ownership, the stores and the OP modes are k_mct_inv_dcshift_planar /
// _pixels' (sYCC at three components only).  NC = 3 / 4: that many
// components, known at compile time; NC = 0: ncomp of them (1 .. 16), the
// loops over 16 unrolled behind uniform guards so every register index stays
// static -- x_k beyond ncomp is zero and so is the matrix there (MctInv), so a
// guard per four k is enough.
// ---------------------------------------------------------------------------
// P pixels of output component j (dj = row j of the matrix) from the KM inputs
template <int KM, int P>
__device__ __forceinline__ void custom_out(const int32_t (&x)[KM][P], const float *dj, uint32_t n, int32_t off,
                                           int32_t mn, int32_t mx, int32_t (&o)[P]) {
#pragma clang fp contract(off)
    float acc[P];
#pragma unroll
    for (int i = 0; i < P; ++i) acc[i] = 0.0f;
#pragma unroll
    for (int k0 = 0; k0 < KM; k0 += 4) {
        if (KM <= 4 || (uint32_t)k0 < n) {
#pragma unroll
            for (int k = k0; k < k0 + 4 && k < KM; ++k) {
                const float d = dj[k];
#pragma unroll
                for (int i = 0; i < P; ++i) acc[i] = __fadd_rn(acc[i], __fmul_rn(d, __int_as_float(x[k][i])));
            }
        }
    }
#pragma unroll
    for (int i = 0; i < P; ++i) {
        const int32_t v = (int32_t)((uint32_t)(int32_t)rintf(acc[i]) + (uint32_t)off);
        o[i] = v < mn ? mn : (v > mx ? mx : v);
    }
}

// a run held as its 16 bytes (4 packed words, low address first), of which the
// first n samples are stored: store_samples' three cases
template <typename T>
__device__ __forceinline__ void store_packed(T *p, const uint32_t (&w)[4], int n) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    constexpr int G = NarrowRun<T>::N, SB = (int)sizeof(T);
    const uintptr_t a = (uintptr_t)p;
    if (n == G && !(a & 15)) {
        const u32x4 q = {w[0], w[1], w[2], w[3]};
        __builtin_nontemporal_store(q, (u32x4 *)p);
    } else if (n == G && !(a & 3)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) __builtin_nontemporal_store(w[j], (uint32_t *)p + j);
    } else {
#pragma unroll
        for (int i = 0; i < G; ++i)
            if (i < n) {
                const uint32_t u = w[i * SB / 4] >> (8 * (i * SB % 4));
                if constexpr (!float_tag<T>) __builtin_nontemporal_store((T)u, p + i);
                else if constexpr (SB == 4) __builtin_nontemporal_store(u, (uint32_t *)p + i);
                else __builtin_nontemporal_store((uint16_t)u, (uint16_t *)p + i);  // (packed: already converted)
            }
    }
}

// planar.  The run is walked in sub-runs of 4 pixels: the 4 x ncomp inputs of
// a sub-run are live together, each output component's 4 samples are packed
// as they are made and shifted into its 16 bytes (pk), so a 16-component
// 8-bit run holds 64 input + 64 packed output registers, not 256 + 256.
template <typename T, int OP = 0, int NC = 0, typename... O>
__global__ void __launch_bounds__(256) k_mct_inv_custom_planar(PlanePtrs src, uint32_t sstride, uint32_t tw, uint32_t th, DstPlanes dst,
                                        uint32_t dstride, uint32_t ncomp, MctInv m, ShiftArr off, ShiftArr minv,
                                        ShiftArr maxv, O... o) {
    static_assert(sizeof...(O) == (OP != 0), "one OutOps exactly when OP != 0");
    static_assert(!op_ycc(OP) || NC == 3, "sYCC / eYCC: three components");
    static_assert(OP != OP_CMYK || NC == 0, "CMYK: the any-count form");
    [[maybe_unused]] const OutOps *const ops = ops_ptr(o...);
    constexpr int N = NarrowRun<T>::N, KM = NC ? NC : GRK_MAX_COMPS;
    constexpr int W = (int)sizeof(T);  // packed words of a sub-run
    const uint32_t nc = NC ? (uint32_t)NC : ncomp;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (y >= th) return;
    const size_t drow = (size_t)y * dstride;
    uint32_t x0;
    const int n = run_of<N>((uintptr_t)((T *)dst.p[0] + drow), sizeof(T), t, tw, x0);
    if (n <= 0) return;
    const size_t si = (size_t)y * sstride + x0, di = drow + x0;
    uint32_t pk[KM][4];
#pragma unroll
    for (int j = 0; j < KM; ++j)
#pragma unroll
        for (int w = 0; w < 4; ++w) pk[j][w] = 0;
    // a sub-run's samples of component j: behind the ones already there
    auto push = [&](uint32_t (&p)[4], const int32_t (&v)[4]) {
#pragma unroll
        for (int w = 0; w + W < 4; ++w) p[w] = p[w + W];
#pragma unroll
        for (int w = 0; w < W; ++w) p[4 - W + w] = pack_word<T>(v, w);
    };
#pragma unroll 1
    for (int s = 0; s < N / 4; ++s) {
        const int left = n - 4 * s, ms = left < 0 ? 0 : (left > 4 ? 4 : left);
        int32_t x[KM][4];
#pragma unroll
        for (int k = 0; k < KM; ++k) {
            if (NC || (uint32_t)k < nc) {
                load_run<4>(src.p[k] + si + 4 * s, ms, x[k]);
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) x[k][i] = 0;
            }
        }
        if constexpr (NC != 0) {
            int32_t v[NC][4];
#pragma unroll
            for (int j = 0; j < NC; ++j)
                custom_out<KM, 4>(x, m.d + j * GRK_MAX_COMPS, nc, off.v[j], minv.v[j], maxv.v[j], v[j]);
            if constexpr (op_ycc(OP)) ycc_run<OP, 4>(v[0], v[1], v[2], *ops);
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                if constexpr (OP != 0) prec_run<4>(v[j], ops->pc[j]);
                push(pk[j], v[j]);
            }
        } else if constexpr (OP == OP_CMYK) {  // (nc >= 4) the four inks together, then channel j - 1 from output j
            int32_t q[4][4];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                custom_out<KM, 4>(x, m.d + j * GRK_MAX_COMPS, nc, off.v[j], minv.v[j], maxv.v[j], q[j]);
            cmyk_run<4>(q[0], q[1], q[2], q[3], *ops);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                prec_run<4>(q[j], ops->pc[j]);
                push(pk[j], q[j]);
            }
#pragma unroll
            for (int j = 4; j < KM; ++j) {
                if ((uint32_t)j < nc) {
                    int32_t v[4];
                    custom_out<KM, 4>(x, m.d + j * GRK_MAX_COMPS, nc, off.v[j], minv.v[j], maxv.v[j], v);
                    prec_run<4>(v, ops->pc[j - 1]);
                    push(pk[j - 1], v);
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < KM; ++j) {
                if ((uint32_t)j < nc) {
                    int32_t v[4];
                    custom_out<KM, 4>(x, m.d + j * GRK_MAX_COMPS, nc, off.v[j], minv.v[j], maxv.v[j], v);
                    if constexpr (OP != 0) prec_run<4>(v, ops->pc[j]);
                    push(pk[j], v);
                }
            }
        }
    }
    const uint32_t nch = OP == OP_CMYK ? nc - 1 : nc;  // channels stored
#pragma unroll
    for (int j = 0; j < KM; ++j) {
        if (NC || (uint32_t)j < nch) store_packed<T>((T *)dst.p[j] + di, pk[j], n);
    }
}

// interleaved.  NC = 3 / 4: k_mct_inv_dcshift_pixels' runs and store; NC = 0:
// any other component count, one thread per pixel, one store per sample
// (k_mct_inv_dcshift_pixels_any's)
template <typename T, int OP = 0, int NC = 0, typename... O>
__global__ void __launch_bounds__(256) k_mct_inv_custom_pixels(PlanePtrs src, uint32_t sstride, uint32_t tw, uint32_t th, DstPlanes dst,
                                        uint32_t dstride, uint32_t ncomp, MctInv m, ShiftArr off, ShiftArr minv,
                                        ShiftArr maxv, O... o) {
    static_assert(sizeof...(O) == (OP != 0), "one OutOps exactly when OP != 0");
    static_assert(!op_ycc(OP) || NC == 3, "sYCC / eYCC: three components");
    static_assert(OP != OP_CMYK || NC == 0, "CMYK: the any-count form");
    [[maybe_unused]] const OutOps *const ops = ops_ptr(o...);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (y >= th) return;
    if constexpr (NC != 0) {
        constexpr int N = NarrowRun<T>::N;
        T *const drow = (T *)dst.p[0] + (size_t)y * dstride;
        uint32_t x0;
        const int n = run_of<N>((uintptr_t)drow, NC * sizeof(T), t, tw, x0);
        if (n <= 0) return;
        const size_t si = (size_t)y * sstride + x0;
        int32_t x[NC][N], v[NC][N];
#pragma unroll
        for (int k = 0; k < NC; ++k) load_run<N>(src.p[k] + si, n, x[k]);
#pragma unroll
        for (int j = 0; j < NC; ++j)
            custom_out<NC, N>(x, m.d + j * GRK_MAX_COMPS, NC, off.v[j], minv.v[j], maxv.v[j], v[j]);
        if constexpr (op_ycc(OP)) ycc_run<OP, N>(v[0], v[1], v[2], *ops);
        if constexpr (OP != 0) {
#pragma unroll
            for (int k = 0; k < NC; ++k) prec_run<N>(v[k], ops->pc[k]);
        }
        int32_t px[N * NC];
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int k = 0; k < NC; ++k) px[i * NC + k] = v[k][i];
        store_samples<T, N * NC>(drow + (size_t)x0 * NC, px, n * NC);
    } else {
        constexpr int KM = GRK_MAX_COMPS;
        if (t >= tw) return;
        const size_t si = (size_t)y * sstride + t;
        T *const d = (T *)dst.p[0] + (size_t)y * dstride + (size_t)t * ncomp;
        int32_t x[KM][1];
#pragma unroll
        for (int k = 0; k < KM; ++k) x[k][0] = (uint32_t)k < ncomp ? src.p[k][si] : 0;
        if constexpr (OP == OP_CMYK) {  // (ncomp >= 4) pixels of ncomp - 1 channels
            T *const dc = (T *)dst.p[0] + (size_t)y * dstride + (size_t)t * (ncomp - 1);
            int32_t q[4][1];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                custom_out<KM, 1>(x, m.d + j * GRK_MAX_COMPS, ncomp, off.v[j], minv.v[j], maxv.v[j], q[j]);
            cmyk_run<1>(q[0], q[1], q[2], q[3], *ops);
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                prec_run<1>(q[j], ops->pc[j]);
                __builtin_nontemporal_store((T)q[j][0], dc + j);
            }
#pragma unroll
            for (int j = 4; j < KM; ++j) {
                if ((uint32_t)j < ncomp) {
                    int32_t v[1];
                    custom_out<KM, 1>(x, m.d + j * GRK_MAX_COMPS, ncomp, off.v[j], minv.v[j], maxv.v[j], v);
                    prec_run<1>(v, ops->pc[j - 1]);
                    __builtin_nontemporal_store((T)v[0], dc + (j - 1));
                }
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < KM; ++j) {
            if ((uint32_t)j < ncomp) {
                int32_t v[1];
                custom_out<KM, 1>(x, m.d + j * GRK_MAX_COMPS, ncomp, off.v[j], minv.v[j], maxv.v[j], v);
                if constexpr (OP != 0) prec_run<1>(v, ops->pc[j]);
                __builtin_nontemporal_store((T)v[0], d + j);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// The JP2 palette and channel order in the last store: jp2_apply_pclr
// (jp2.cpp:1301-1407) and the channel swaps of jp2_apply_cdef (:1564-1623),
// which the reference runs as CPU passes over the decoded int32 planes, applied
// to the run values k_mct_inv_dcshift_planar / _pixels hold.  A component is
// finished by the existing statements (inverse MCT, DC shift, clamp); then
// output channel c, fed by component map.comp[c], receives
//     map.pcol[c] < 0:  the component's sample                    (direct use)
//     otherwise:        table[clamp(sample, 0, ne - 1) * npc + map.pcol[c]]
// The cdef swaps are already folded into map on the host.  Channels and
// components differ in number (1 -> 3, 2 -> 4, ...): a lane reads a
// component's run once and stores every channel it feeds.
//
// The table (ne x npc entries of 16 bits, at most 1024 x 16 = 32 KB) lives in
// LDS: each workgroup copies it from the device table before its first run
// and keeps it for PAL_ROWS rows, so a full-size table costs 4 B of LDS fill
// per 1 B of 8-bit index at worst and a 256 x 3 one 0.05 B.  map.zero: the
// components are not read and count as finished zero samples (the fill of a
// tile the stream never reached: entry 0, as the reference's pass over its
// zero planes gives).  Run ownership, stores and the precision ops are the
// existing kernels'.
// ---------------------------------------------------------------------------
constexpr int PAL_ROWS = 8;

__device__ __forceinline__ void palette_load(uint16_t *lut, const uint16_t *table, uint32_t n) {
    if (!((uintptr_t)table & 3)) {
        for (uint32_t i = threadIdx.x; i < n / 2; i += blockDim.x) ((uint32_t *)lut)[i] = ((const uint32_t *)table)[i];
        if ((n & 1) && threadIdx.x == 0) lut[n - 1] = table[n - 1];
    } else {
        for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) lut[i] = table[i];
    }
    __syncthreads();
}

// the table rows a finished run indexes: clamp(sample, 0, ne - 1) * npc, made
// once per sample for every channel the component feeds
template <int N>
__device__ __forceinline__ void palette_rows(const int32_t (&a)[N], const PalMap &map, uint32_t (&row)[N]) {
    const int32_t top = (int32_t)map.ne - 1;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const int32_t k = a[i] < 0 ? 0 : (a[i] > top ? top : a[i]);
        row[i] = map.ne ? (uint32_t)k * map.npc : 0u;
    }
}

// one channel's values from its component's finished run and rows
template <int N>
__device__ __forceinline__ void palette_run(const int32_t (&a)[N], const uint32_t (&row)[N], int32_t pcol,
                                            const uint16_t *lut, int32_t (&o)[N]) {
    if (pcol < 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = a[i];
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) o[i] = lut[row[i] + (uint32_t)pcol];
    }
}

// load_run, also for the one-sample "run" of the thread-per-pixel path (whose
// wide branch would load nothing)
template <int N>
__device__ __forceinline__ void pal_load(const int32_t *p, int n, int32_t (&v)[N]) {
    if constexpr (N >= 4) {
        load_run<N>(p, n, v);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = i < n ? p[i] : 0;
    }
}

// The finished runs of the components that feed a channel, one after the
// other, each handed to emit(component, run): the MCT triple first.  KMAX as
// in the store bodies above: GRK_MAX_COMPS for kernel arguments, indexed at run
// time, or 4 for a PalJob's, which sit in scalar registers (static indices
// behind uniform guards).
template <int N, int KMAX = GRK_MAX_COMPS, typename F>
__device__ __forceinline__ void palette_components(const PlanePtrs &src, size_t si, int n, uint32_t ncomp,
                                                   const ShiftArr &shift, const ShiftArr &minv, const ShiftArr &maxv,
                                                   int32_t mct, int32_t irrev, const PalMap &map, F emit) {
    uint32_t k0 = 0;
    if (mct && ncomp >= 3) {
        int32_t a[N], b[N], c[N];
        if (!map.zero) {
            pal_load<N>(src.p[0] + si, n, a);
            pal_load<N>(src.p[1] + si, n, b);
            pal_load<N>(src.p[2] + si, n, c);
            inv_mct_run<N>(a, b, c, irrev, shift, minv, maxv);
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) a[i] = b[i] = c[i] = 0;
        }
        uint32_t row[N];
        palette_rows<N>(a, map, row);
        emit(0u, a, row);
        palette_rows<N>(b, map, row);
        emit(1u, b, row);
        palette_rows<N>(c, map, row);
        emit(2u, c, row);
        k0 = 3;
    }
    const auto plain = [&](uint32_t k) {
        if (!((map.used >> k) & 1)) return;  // feeds no channel
        int32_t a[N];
        if (!map.zero) {
            pal_load<N>(src.p[k] + si, n, a);
            inv_plain_run<N>(a, (irrev >> k) & 1, shift.v[k], minv.v[k], maxv.v[k]);
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) a[i] = 0;
        }
        uint32_t row[N];
        palette_rows<N>(a, map, row);
        emit(k, a, row);
    };
    if constexpr (KMAX > 4) {
        for (uint32_t k = k0; k < ncomp; ++k) plain(k);
    } else {
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
            if ((uint32_t)k >= k0 && (uint32_t)k < ncomp) plain((uint32_t)k);
    }
}

// f(c) for every channel c < nch: a run-time loop, or (KMAX = 4) unrolled behind uniform guards
template <int KMAX, typename F>
__device__ __forceinline__ void palette_channels(uint32_t nch, F f) {
    if constexpr (KMAX > 4) {
        for (uint32_t c = 0; c < nch; ++c) f(c);
    } else {
#pragma unroll
        for (int c = 0; c < KMAX; ++c)
            if ((uint32_t)c < nch) f((uint32_t)c);
    }
}

// The bodies of the palette stores, shared by the per-tile kernels and the
// job-table kernel k_palette_jobs below: thread t of row y finishes its run
// (or pixel), looks it up in the workgroup's LDS table `lut` and stores it.
// Every argument but t is uniform over the workgroup; ops: null exactly when
// OP = 0; KMAX as in palette_components.
//
// planar: dst.p[c] = plane of channel c
template <typename T, int OP, int KMAX = GRK_MAX_COMPS>
__device__ __forceinline__ void palette_planar_row(const PlanePtrs &src, uint32_t sstride, uint32_t tw,
                                                   const DstPlanes &dst, uint32_t dstride, uint32_t ncomp, uint32_t y,
                                                   uint32_t t, const ShiftArr &shift, const ShiftArr &minv,
                                                   const ShiftArr &maxv, int32_t mct, int32_t irrev, const PalMap &map,
                                                   const uint16_t *lut, [[maybe_unused]] const OutOps *ops) {
    constexpr int N = NarrowRun<T>::N;
    const size_t drow = (size_t)y * dstride;
    uint32_t x0;
    const int n = run_of<N>((uintptr_t)((T *)dst.p[0] + drow), sizeof(T), t, tw, x0);
    if (n <= 0) return;
    const size_t si = (size_t)y * sstride + x0, di = drow + x0;
    palette_components<N, KMAX>(src, si, n, ncomp, shift, minv, maxv, mct, irrev, map,
                                [&](uint32_t k, const int32_t (&a)[N], const uint32_t (&row)[N]) {
                                    palette_channels<KMAX>(map.nch, [&](uint32_t c) {
                                        if (map.comp[c] != k) return;
                                        int32_t v[N];
                                        palette_run<N>(a, row, map.pcol[c], lut, v);
                                        if constexpr (OP != 0) prec_run<N>(v, ops->pc[c]);
                                        store_samples<T, N>((T *)dst.p[c] + di, v, n);
                                    });
                                });
}

// interleaved, NCH = 3 / 4 channels: channel c of pixel (y, x) at
// dst0[y * dstride + x * NCH + c], runs on the destination's 16-byte grid
template <typename T, int NCH, int OP, int KMAX = GRK_MAX_COMPS>
__device__ __forceinline__ void palette_pixels_row(const PlanePtrs &src, uint32_t sstride, uint32_t tw, void *dst0,
                                                   uint32_t dstride, uint32_t ncomp, uint32_t y, uint32_t t,
                                                   const ShiftArr &shift, const ShiftArr &minv, const ShiftArr &maxv,
                                                   int32_t mct, int32_t irrev, const PalMap &map, const uint16_t *lut,
                                                   [[maybe_unused]] const OutOps *ops) {
    constexpr int N = NarrowRun<T>::N;
    T *const drow = (T *)dst0 + (size_t)y * dstride;
    uint32_t x0;
    const int n = run_of<N>((uintptr_t)drow, NCH * sizeof(T), t, tw, x0);
    if (n <= 0) return;
    const size_t si = (size_t)y * sstride + x0;
    int32_t v[NCH][N];
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int i = 0; i < N; ++i) v[c][i] = 0;
    palette_components<N, KMAX>(src, si, n, ncomp, shift, minv, maxv, mct, irrev, map,
                                [&](uint32_t k, const int32_t (&a)[N], const uint32_t (&row)[N]) {
#pragma unroll
                                    for (int c = 0; c < NCH; ++c)
                                        if (map.comp[c] == k) palette_run<N>(a, row, map.pcol[c], lut, v[c]);
                                });
    if constexpr (OP != 0) {
#pragma unroll
        for (int c = 0; c < NCH; ++c) prec_run<N>(v[c], ops->pc[c]);
    }
    int32_t px[N * NCH];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int c = 0; c < NCH; ++c) px[i * NCH + c] = v[c][i];
    store_samples<T, N * NCH>(drow + (size_t)x0 * NCH, px, n * NCH);
}

// interleaved, any other channel count: pixel x of row y, one store per sample
template <typename T, int OP, int KMAX = GRK_MAX_COMPS>
__device__ __forceinline__ void palette_pixel_any(const PlanePtrs &src, uint32_t sstride, uint32_t tw, void *dst0,
                                                  uint32_t dstride, uint32_t ncomp, uint32_t y, uint32_t x,
                                                  const ShiftArr &shift, const ShiftArr &minv, const ShiftArr &maxv,
                                                  int32_t mct, int32_t irrev, const PalMap &map, const uint16_t *lut,
                                                  [[maybe_unused]] const OutOps *ops) {
    if (x >= tw) return;
    const size_t si = (size_t)y * sstride + x;
    T *const d = (T *)dst0 + (size_t)y * dstride + (size_t)x * map.nch;
    palette_components<1, KMAX>(src, si, 1, ncomp, shift, minv, maxv, mct, irrev, map,
                                [&](uint32_t k, const int32_t (&a)[1], const uint32_t (&row)[1]) {
                                    palette_channels<KMAX>(map.nch, [&](uint32_t c) {
                                        if (map.comp[c] != k) return;
                                        int32_t v[1];
                                        palette_run<1>(a, row, map.pcol[c], lut, v);
                                        if constexpr (OP != 0) prec_run<1>(v, ops->pc[c]);
                                        __builtin_nontemporal_store((T)v[0], d + c);
                                    });
                                });
}

// The per-tile kernels: a (row threads, bands of PAL_ROWS rows) grid in front
// of those bodies.
// planar: dst.p[c] = plane of channel c
template <typename T, int OP = 0, typename... O>
__global__ void __launch_bounds__(256) k_palette_planar(PlanePtrs src, uint32_t sstride, uint32_t tw, uint32_t th,
                                                        DstPlanes dst, uint32_t dstride, uint32_t ncomp,
                                                        ShiftArr shift, ShiftArr minv, ShiftArr maxv, int32_t mct,
                                                        int32_t irrev, PalMap map, const uint16_t *table, O... o) {
    static_assert(sizeof...(O) == (OP != 0), "one OutOps exactly when OP != 0");
    static_assert(OP == 0 || OP == OP_PREC, "no colour conversion behind a palette");
    const OutOps *const ops = ops_ptr(o...);
    extern __shared__ uint16_t pal_lut[];
    palette_load(pal_lut, table, map.ne * map.npc);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t yb = blockIdx.y * PAL_ROWS, ye = yb + PAL_ROWS < th ? yb + PAL_ROWS : th;
    for (uint32_t y = yb; y < ye; ++y)
        palette_planar_row<T, OP>(src, sstride, tw, dst, dstride, ncomp, y, t, shift, minv, maxv, mct, irrev, map,
                                  pal_lut, ops);
}

// interleaved: channel c of pixel (y, x) at dst.p[0][y * dstride + x * nch + c].
// NCH = 3 / 4: that many channels, runs on the destination's 16-byte grid;
// NCH = 0: map.nch of them, one thread per pixel, one store per sample
template <typename T, int NCH, int OP = 0, typename... O>
__global__ void __launch_bounds__(256) k_palette_pixels(PlanePtrs src, uint32_t sstride, uint32_t tw, uint32_t th,
                                                        DstPlanes dst, uint32_t dstride, uint32_t ncomp,
                                                        ShiftArr shift, ShiftArr minv, ShiftArr maxv, int32_t mct,
                                                        int32_t irrev, PalMap map, const uint16_t *table, O... o) {
    static_assert(sizeof...(O) == (OP != 0), "one OutOps exactly when OP != 0");
    static_assert(OP == 0 || OP == OP_PREC, "no colour conversion behind a palette");
    const OutOps *const ops = ops_ptr(o...);
    extern __shared__ uint16_t pal_lut[];
    palette_load(pal_lut, table, map.ne * map.npc);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t yb = blockIdx.y * PAL_ROWS, ye = yb + PAL_ROWS < th ? yb + PAL_ROWS : th;
    for (uint32_t y = yb; y < ye; ++y) {
        if constexpr (NCH != 0)
            palette_pixels_row<T, NCH, OP>(src, sstride, tw, dst.p[0], dstride, ncomp, y, t, shift, minv, maxv, mct,
                                           irrev, map, pal_lut, ops);
        else
            palette_pixel_any<T, OP>(src, sstride, tw, dst.p[0], dstride, ncomp, y, t, shift, minv, maxv, mct, irrev, map,
                                     pal_lut, ops);
    }
}

// ---------------------------------------------------------------------------
// The decoded image with its subsampled components replicated to the image
// grid (GRKGPU_LAYOUT_UPSAMPLE; grk_decompress -u, upsample_image_components,
// grk_decompress.cpp:891-1040): output pixel (X, Y) of the reference grid
// takes component k's sample (floor(X / dx) - gx0, floor(Y / dy) - gy0) -- zero
// where that index is negative, the reference's lead-in when the origin is no
// multiple of dx / dy.  A component comes straight from the tile buffer
// (UpComp::raw: k_mct_inv_dcshift's second loop, statement for statement) or,
// where a tile's first pixels map to a sample of the neighbouring tile or the
// MCT ran first, from its finished staging plane, which spans the tile seams;
// the stores are k_mct_inv_dcshift_planar / _pixels'.
// ---------------------------------------------------------------------------
// component c's sample for the pixel whose column / row on c's grid are (col, row)
// a finished (not raw) sample: of the destination's type T, or (OP != 0) of the
// format the component carries (UPCOMP_FIN + SampleFmt, uniform over the launch)
template <typename T, int OP>
__device__ __forceinline__ int32_t fin_sample(const UpComp &c, size_t i) {
    if constexpr (OP == 0) {
        return (int32_t)((const T *)c.src)[i];
    } else {
        switch (c.raw - UPCOMP_FIN) {
            case SMP_U8: return (int32_t)((const uint8_t *)c.src)[i];
            case SMP_I8: return (int32_t)((const int8_t *)c.src)[i];
            case SMP_U16: return (int32_t)((const uint16_t *)c.src)[i];
            case SMP_I16: return (int32_t)((const int16_t *)c.src)[i];
            default: return ((const int32_t *)c.src)[i];
        }
    }
}
template <int OP>
__device__ __forceinline__ bool is_raw(const UpComp &c) {
    if constexpr (OP == 0) return c.raw;
    else return c.raw == 1;
}

template <typename T, int OP = 0>
__device__ __forceinline__ int32_t up_sample(const UpComp &c, int32_t col, int32_t row) {
    if (col < c.zx0 || row < c.zy0 || !c.src) return 0;
    const size_t i = (size_t)(row - c.gy0) * c.stride + (uint32_t)(col - c.gx0);
    if (is_raw<OP>(c)) {
        int32_t a[1] = {((const int32_t *)c.src)[i]};
        inv_plain_run<1>(a, c.irrev, c.shift, c.mn, c.mx);
        return a[0];
    }
    return fin_sample<T, OP>(c, i);
}

// 4:2:0 / 4:2:2: three components at (1,1), (2,dy), (2,dy), dy = 1 or 2.  A
// thread owns the run of N pixels k_mct_inv_dcshift_planar / _pixels give it
// (16 bytes of a destination row per component, on the destination's 16-byte
// grid; lead-in and cut last run sample by sample).  The run's chroma is the
// N / 2 (+ 1 when the run starts on an odd X) source samples from floor(X / 2)
// on, each stored twice: what counts is the parity of the absolute X, not of
// the run's place in the tile.  Row Y reads chroma row floor(Y / dy).
//
// OP != 0 (OutOps): the sYCC chroma terms are computed once per source sample
// (NS pairs), not per pixel, and replicated like the samples themselves.
//
// upsample_420_run is thread t of row y (pc = the three components, dstp = the
// destination planes, both uniform): the body of k_upsample_420, and of the
// job-table kernel k_conv_jobs_420.
template <typename T, bool IL, int OP>
__device__ __forceinline__ void upsample_420_run(const UpComp *pc, uint32_t X0, uint32_t Y0, uint32_t w, uint32_t t,
                                                 uint32_t y, void *const *dstp, uint32_t dstride,
                                                 [[maybe_unused]] const OutOps *ops) {
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    constexpr int N = NarrowRun<T>::N, H = N / 2, NS = H + 1;
    const size_t drow = (size_t)y * dstride;
    uint32_t x0;
    const int n = run_of<N>((uintptr_t)((T *)dstp[0] + drow), (IL ? 3 : 1) * sizeof(T), t, w, x0);
    if (n <= 0) return;
    const uint32_t X = X0 + x0, Y = Y0 + y;
    int32_t v[3][N];
    {
        const UpComp &c = pc[0];  // (1,1): every pixel has its sample
        const size_t si = (size_t)(Y - (uint32_t)c.gy0) * c.stride + (X - (uint32_t)c.gx0);
        if (!c.src) {
#pragma unroll
            for (int i = 0; i < N; ++i) v[0][i] = 0;
        } else if (OP ? c.raw == 1 : c.raw) {
            load_run<N>((const int32_t *)c.src + si, n, v[0]);
            inv_plain_run<N>(v[0], c.irrev, c.shift, c.mn, c.mx);
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                if constexpr (OP == 0) v[0][i] = i < n ? (int32_t)((const T *)c.src)[si + i] : 0;
                else v[0][i] = i < n ? fin_sample<T, OP>(c, si + i) : 0;
            }
        }
    }
    int32_t cs[2][NS];  // (sYCC: the chroma samples of the run, Cb and Cr)
    const int32_t c0 = (int32_t)(X >> 1);                             // the run's first chroma column
    const int last = (int)(((X + (uint32_t)n - 1) >> 1) - (X >> 1));  // ... and how many more it needs
    const bool odd = X & 1;
#pragma unroll
    for (int k = 1; k < 3; ++k) {
        const UpComp &c = pc[k];
        const int32_t row = (int32_t)(Y >> (c.dy - 1));
        int32_t s[NS];
        if (row < c.zy0 || !c.src) {
#pragma unroll
            for (int j = 0; j < NS; ++j) s[j] = 0;
        } else if (OP ? c.raw == 1 : c.raw) {
            const int32_t *const q = (const int32_t *)c.src + ((int64_t)(row - c.gy0) * c.stride + (c0 - c.gx0));
            if (H % 4 == 0 && n == N && c0 >= c.zx0 && !((uintptr_t)q & 15)) {
#pragma unroll
                for (int g = 0; g < H / 4; ++g) {
                    const i32x4 u = ((const i32x4 *)q)[g];
                    s[4 * g] = u.x; s[4 * g + 1] = u.y; s[4 * g + 2] = u.z; s[4 * g + 3] = u.w;
                }
                s[H] = odd ? q[H] : 0;
                inv_plain_run<NS>(s, c.irrev, c.shift, c.mn, c.mx);
            } else {
#pragma unroll
                for (int j = 0; j < NS; ++j) s[j] = c0 + j >= c.zx0 && j <= last ? q[j] : 0;
                inv_plain_run<NS>(s, c.irrev, c.shift, c.mn, c.mx);
#pragma unroll
                for (int j = 0; j < NS; ++j) s[j] = c0 + j >= c.zx0 ? s[j] : 0;  // the zero lead-in
            }
        } else {
            const int64_t b = (int64_t)(row - c.gy0) * c.stride + (c0 - c.gx0);
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                if constexpr (OP == 0) s[j] = c0 + j >= c.zx0 && j <= last ? (int32_t)((const T *)c.src)[b + j] : 0;
                else s[j] = c0 + j >= c.zx0 && j <= last ? fin_sample<T, OP>(c, (size_t)(b + j)) : 0;
            }
        }
        if constexpr (OP == OP_SYCC) {
#pragma unroll
            for (int j = 0; j < NS; ++j) cs[k - 1][j] = s[j];
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) v[k][i] = odd ? s[(i + 1) >> 1] : s[i >> 1];
        }
    }
    if constexpr (OP == OP_SYCC) {
        int32_t tr[NS], tg[NS], tb[NS];
#pragma unroll
        for (int j = 0; j < NS; ++j) sycc_terms(cs[0][j], cs[1][j], ops->off, tr[j], tg[j], tb[j]);
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const int j0 = i >> 1, j1 = (i + 1) >> 1;
            sycc_pixel(v[0][i], odd ? tr[j1] : tr[j0], odd ? tg[j1] : tg[j0], odd ? tb[j1] : tb[j0], ops->upb,
                       v[0][i], v[1][i], v[2][i]);
        }
    }
    if constexpr (OP != 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            prec_run<N>(v[k], ops->pc[k]);
            norm_run<T, N>(v[k], *ops, k);
        }
    }
    if constexpr (IL) {
        int32_t px[N * 3];
#pragma unroll
        for (int i = 0; i < N; ++i)
#pragma unroll
            for (int k = 0; k < 3; ++k) px[i * 3 + k] = v[k][i];
        store_samples<T, N * 3>((T *)dstp[0] + drow + (size_t)x0 * 3, px, n * 3);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) store_samples<T, N>((T *)dstp[k] + drow + x0, v[k], n);
    }
}

template <typename T, bool IL, int OP = 0, typename... O>
__global__ void k_upsample_420(UpPlan p, uint32_t X0, uint32_t Y0, uint32_t w, uint32_t h, DstPlanes dst,
                               uint32_t dstride, O... o) {
    static_assert(sizeof...(O) == (OP != 0), "one OutOps exactly when OP != 0");
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (y >= h) return;
    upsample_420_run<T, IL, OP>(p.c, X0, Y0, w, t, y, dst.p, dstride, ops_ptr(o...));
}

// any component count and any dx / dy in 1 .. 255: one thread per pixel, one store per sample.
// OP != 0 (one OutOps in the pack): the precision op of each component, and
// sYCC (ops.sycc, three components -- the shapes k_upsample_420 does not take:
// chroma at (1,1) fed finished samples, and the converted value of samples
// nothing decoded) at run time.
//
// upsample_any_pixel is pixel (x, y) of the rectangle (pc = the components,
// dstp = the destination planes, both uniform): the body of k_upsample_any,
// and of the job-table kernel k_conv_jobs_any.
template <typename T, int OP>
__device__ __forceinline__ void upsample_any_pixel(const UpComp *pc, uint32_t ncomp, uint32_t X0, uint32_t Y0,
                                                   uint32_t x, uint32_t y, void *const *dstp, int32_t il,
                                                   uint32_t dstride, [[maybe_unused]] const OutOps *ops) {
    const uint32_t X = X0 + x, Y = Y0 + y;
    const size_t drow = (size_t)y * dstride;
    if constexpr (OP != 0) {
        if (ops->sycc) {
            int32_t v[3][1];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                v[k][0] = up_sample<T, OP>(pc[k], (int32_t)(X / pc[k].dx), (int32_t)(Y / pc[k].dy));
            sycc_run<1>(v[0], v[1], v[2], *ops);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                prec_run<1>(v[k], ops->pc[k]);
                norm_run<T, 1>(v[k], *ops, k);
                T *const d = il ? (T *)dstp[0] + drow + (size_t)x * 3 + k : (T *)dstp[k] + drow + x;
                store_sample<T>(v[k][0], d);
            }
            return;
        }
        if (ops->col == COL_EYCC) {  // (three components, one grid)
            int32_t v[3][1];
#pragma unroll
            for (int k = 0; k < 3; ++k)
                v[k][0] = up_sample<T, OP>(pc[k], (int32_t)(X / pc[k].dx), (int32_t)(Y / pc[k].dy));
            eycc_run<1>(v[0], v[1], v[2], *ops);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                prec_run<1>(v[k], ops->pc[k]);
                norm_run<T, 1>(v[k], *ops, k);
                T *const d = il ? (T *)dstp[0] + drow + (size_t)x * 3 + k : (T *)dstp[k] + drow + x;
                store_sample<T>(v[k][0], d);
            }
            return;
        }
        if (ops->col == COL_CMYK) {  // (ncomp >= 4 components, ncomp - 1 channels)
            int32_t v[4][1];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                v[k][0] = up_sample<T, OP>(pc[k], (int32_t)(X / pc[k].dx), (int32_t)(Y / pc[k].dy));
            cmyk_run<1>(v[0], v[1], v[2], v[3], *ops);
            for (uint32_t ch = 0; ch + 1 < ncomp; ++ch) {
                int32_t a[1];
                if (ch < 3) {
                    a[0] = ch == 0 ? v[0][0] : (ch == 1 ? v[1][0] : v[2][0]);
                } else {
                    const UpComp &c = pc[ch + 1];
                    a[0] = up_sample<T, OP>(c, (int32_t)(X / c.dx), (int32_t)(Y / c.dy));
                }
                prec_run<1>(a, ops->pc[ch]);
                norm_run<T, 1>(a, *ops, ch);
                T *const d = il ? (T *)dstp[0] + drow + (size_t)x * (ncomp - 1) + ch : (T *)dstp[ch] + drow + x;
                store_sample<T>(a[0], d);
            }
            return;
        }
    }
    for (uint32_t k = 0; k < ncomp; ++k) {
        const UpComp &c = pc[k];
        if constexpr (OP == 0) {
            const int32_t v = up_sample<T>(c, (int32_t)(X / c.dx), (int32_t)(Y / c.dy));
            T *const d = il ? (T *)dstp[0] + drow + (size_t)x * ncomp + k : (T *)dstp[k] + drow + x;
            __builtin_nontemporal_store((T)v, d);
        } else {
            int32_t v[1] = {up_sample<T, OP>(c, (int32_t)(X / c.dx), (int32_t)(Y / c.dy))};
            prec_run<1>(v, ops->pc[k]);
            norm_run<T, 1>(v, *ops, k);
            T *const d = il ? (T *)dstp[0] + drow + (size_t)x * ncomp + k : (T *)dstp[k] + drow + x;
            store_sample<T>(v[0], d);
        }
    }
}
template <typename T, int OP = 0, typename... O>
__global__ void k_upsample_any(UpPlan p, uint32_t ncomp, uint32_t X0, uint32_t Y0, uint32_t w, uint32_t h,
                               DstPlanes dst, int32_t il, uint32_t dstride, O... o) {
    static_assert(sizeof...(O) == (OP != 0), "one OutOps exactly when OP != 0");
    const uint32_t x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= w || y >= h) return;
    upsample_any_pixel<T, OP>(p.c, ncomp, X0, Y0, x, y, dst.p, il, dstride, ops_ptr(o...));
}

// ---------------------------------------------------------------------------
// DC shift + forward MCT from the layouts a producer of frames holds: pixel-
// interleaved samples (image loaders, video capture, the PPM raster) and
// big-endian 16-bit samples (the 16-bit PGM / PPM raster) -- the mirror image
// of the narrowing decode kernels above.  k_dcshift_mct_fwd's arithmetic,
// statement for statement; only the loads differ.
// ---------------------------------------------------------------------------
// the 4 / sizeof(S) samples of one loaded dword, low address first; a
// big-endian dword's two samples are put right by one v_perm_b32
template <typename S, bool BE>
__device__ __forceinline__ void unpack_word(uint32_t w, int32_t *o) {
    if constexpr (sizeof(S) == 4) {
        o[0] = (int32_t)w;
    } else if constexpr (sizeof(S) == 2) {
        if constexpr (BE) w = __builtin_amdgcn_perm(w, w, 0x02030001u);
        o[0] = (int32_t)(S)(w & 0xffffu);
        o[1] = (int32_t)(S)(w >> 16);
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = (int32_t)(S)((w >> (8 * i)) & 0xffu);
    }
}

// NS samples (a whole number of dwords) of which the first n are read: as
// dwordx4 where p is 16-byte aligned, dwordx2 where 8-byte aligned, dwords
// where 4-byte aligned (as far as the run's size divides), single samples
// otherwise
template <typename S, int NS, bool BE>
__device__ __forceinline__ void load_samples(const uint8_t *p, int32_t (&v)[NS], int n) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
    constexpr int BYTES = NS * (int)sizeof(S);
    constexpr int W = 4 / (int)sizeof(S);  // samples per dword
    static_assert(BYTES % 4 == 0, "a run is a whole number of dwords");
    const uintptr_t a = (uintptr_t)p;
    if (BYTES % 16 == 0 && n == NS && !(a & 15)) {
#pragma unroll
        for (int g = 0; g < BYTES / 16; ++g) {
            const u32x4 q = ((const u32x4 *)p)[g];
            unpack_word<S, BE>(q.x, v + g * 4 * W);
            unpack_word<S, BE>(q.y, v + g * 4 * W + W);
            unpack_word<S, BE>(q.z, v + g * 4 * W + 2 * W);
            unpack_word<S, BE>(q.w, v + g * 4 * W + 3 * W);
        }
    } else if (BYTES % 8 == 0 && n == NS && !(a & 7)) {
#pragma unroll
        for (int g = 0; g < BYTES / 8; ++g) {
            const u32x2 q = ((const u32x2 *)p)[g];
            unpack_word<S, BE>(q.x, v + g * 2 * W);
            unpack_word<S, BE>(q.y, v + g * 2 * W + W);
        }
    } else if (n == NS && !(a & 3)) {
#pragma unroll
        for (int j = 0; j < BYTES / 4; ++j) unpack_word<S, BE>(((const uint32_t *)p)[j], v + j * W);
    } else {
#pragma unroll
        for (int i = 0; i < NS; ++i) v[i] = i < n ? ld_sample<S, BE>(p + (size_t)i * sizeof(S)) : 0;
    }
}

// the run of thread t of a source row at byte address a whose pixels are pxb
// bytes (run_of's layout: thread 0 takes the `lead` pixels before the grid,
// thread t > 0 the run from lead + (t - 1) * N, the last run cut at tw), the
// grid laid where the runs are best aligned: on a 16-byte boundary if one is
// within a run's length, else an 8-, else a 4-byte one
template <int N>
__device__ __forceinline__ int src_run_of(uintptr_t a, uint32_t pxb, uint32_t t, uint32_t tw, uint32_t &x0) {
    uint32_t lead = 0;
    bool found = false;
#pragma unroll
    for (uint32_t al = 16; al >= 4; al >>= 1)
#pragma unroll
        for (uint32_t l = 0; l < (uint32_t)N; ++l)
            if (!found && !((a + (uintptr_t)l * pxb) & (al - 1))) { lead = l; found = true; }
    const uint64_t first = t ? (uint64_t)lead + (uint64_t)(t - 1) * N : 0;
    const uint64_t end = t ? first + N : lead;
    x0 = (uint32_t)(first < tw ? first : tw);
    return (int)((end < tw ? end : tw) - x0);
}

// n <= N int32 results of one component's row
template <int N>
__device__ __forceinline__ void store_run(int32_t *p, const int32_t (&v)[N], int n) {
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    if (n == N && !((uintptr_t)p & 15)) {
#pragma unroll
        for (int g = 0; g < N / 4; ++g) {
            const i32x4 q = {v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
            __builtin_nontemporal_store(q, (i32x4 *)p + g);
        }
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i)
            if (i < n) put<true>(p + i, v[i]);
    }
}

// M: bit 0 = big-endian samples, bit 1 = interleaved (sample (y, x, c) at
// src.p[0][y * sstride + x * ncomp + c]; else planar, src.p[c][y * sstride +
// x]).  One thread per sample position, one load per component, any byte
// alignment; dst rows dstride apart.
template <typename S, int M>
__global__ void k_dcshift_mct_fwd_from(SrcPlanes src, uint32_t sstride, PlanePtrs dst, uint32_t dstride, uint32_t tw,
                                       uint32_t th, uint32_t ncomp, ShiftArr shift, int32_t mct, int32_t irrev) {
    uint32_t x = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t y = blockIdx.y;
    if (x >= tw || y >= th) return;
    const size_t srow = (size_t)y * sstride, di = (size_t)y * dstride + x;
    auto smp = [&](uint32_t c) {
        const uint8_t *p = (M & 2) ? (const uint8_t *)src.p[0] + (srow + (size_t)x * ncomp + c) * sizeof(S)
                                   : (const uint8_t *)src.p[c] + (srow + x) * sizeof(S);
        return ld_sample<S, (M & 1) != 0>(p);
    };
    uint32_t c0 = 0;
    if (mct && ncomp >= 3) {
        int32_t r = smp(0) - shift.v[0], g = smp(1) - shift.v[1], b = smp(2) - shift.v[2];
        int32_t o0, o1, o2;
        if (!irrev) {
            o0 = (r + (g * 2) + b) >> 2;
            o1 = b - g;
            o2 = r - g;
        } else {
            o0 = ict_term(r, 2449) + ict_term(g, 4809) + ict_term(b, 934);
            o1 = -ict_term(r, 1382) - ict_term(g, 2714) + ict_term(b, 4096);
            o2 = ict_term(r, 4096) - ict_term(g, 3430) - ict_term(b, 666);
        }
        put<true>(&dst.p[0][di], o0); put<true>(&dst.p[1][di], o1); put<true>(&dst.p[2][di], o2);
        c0 = 3;
    }
    for (uint32_t c = c0; c < ncomp; ++c) {
        int32_t v = smp(c) - shift.v[c];
        put<true>(&dst.p[c][di], irrev ? (int32_t)((uint32_t)v << 11) : v);
    }
}

// Interleaved, NC = 3 or 4 components.  A thread owns a run of PIX_RUN = 4
// adjacent pixels of one row: it reads the run's 4 * NC contiguous samples
// with the widest loads their address allows (load_samples), unpacks them,
// applies the DC shift + RCT / ICT, and stores each component's run to its
// int32 tile buffer as ONE non-temporal dwordx4, so every store instruction of
// a wavefront writes whole lines -- two thirds of this pass's bytes are its
// stores.  (Runs of 16 / sizeof(S) pixels, the narrowing decode kernel's, were
// measured first: a lane then stores two / four dwordx4 per component, 32 / 64
// bytes from its neighbour's, each instruction covering half / a quarter of
// every line it touches -- 0.176 ms for the 8K 12-bit uint16 frame against
// 0.125 planar and 0.118 with runs of 4)  Runs lie on the best
// aligned grid of the source row (src_run_of: thread 0 takes the pixels before
// it, the last run is cut at tw), so any byte offset, column origin and row
// stride is correct and the aligned interior is fast.
constexpr int PIX_RUN = 4;
template <typename S, int NC, bool BE>
__global__ __launch_bounds__(256) void k_dcshift_mct_fwd_pixels(SrcPlanes src, uint32_t sstride, PlanePtrs dst, uint32_t dstride, uint32_t tw,
                                         uint32_t th, ShiftArr shift, int32_t mct, int32_t irrev) {
    constexpr int N = PIX_RUN;
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (y >= th) return;
    const uint8_t *const srow = (const uint8_t *)src.p[0] + (size_t)y * sstride * sizeof(S);
    uint32_t x0;
    const int n = src_run_of<N>((uintptr_t)srow, NC * sizeof(S), t, tw, x0);
    if (n <= 0) return;
    int32_t px[N * NC];
    load_samples<S, N * NC, BE>(srow + (size_t)x0 * NC * sizeof(S), px, n * NC);
    int32_t v[NC][N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int k = 0; k < NC; ++k) v[k][i] = px[i * NC + k];
    if (mct) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            int32_t r = v[0][i] - shift.v[0], g = v[1][i] - shift.v[1], b = v[2][i] - shift.v[2];
            int32_t o0, o1, o2;
            if (!irrev) {
                o0 = (r + (g * 2) + b) >> 2;
                o1 = b - g;
                o2 = r - g;
            } else {
                o0 = ict_term(r, 2449) + ict_term(g, 4809) + ict_term(b, 934);
                o1 = -ict_term(r, 1382) - ict_term(g, 2714) + ict_term(b, 4096);
                o2 = ict_term(r, 4096) - ict_term(g, 3430) - ict_term(b, 666);
            }
            v[0][i] = o0; v[1][i] = o1; v[2][i] = o2;
        }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        if (mct && k < 3) continue;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            int32_t s = v[k][i] - shift.v[k];
            v[k][i] = irrev ? (int32_t)((uint32_t)s << 11) : s;
        }
    }
    const size_t di = (size_t)y * dstride + x0;
#pragma unroll
    for (int k = 0; k < NC; ++k) store_run<N>(dst.p[k] + di, v[k], n);
}

// ---------------------------------------------------------------------------
// T1 (t1_lane.h).  Encode = prep (wave per block: quantise, sign rows, numbps,
// magnitude bit-planes via ballots) + lane coder (one lane per block).
// Decode = lane decoder (one lane per block, write-only bit-plane rows) +
// rebuild (workgroup per block: values + post-decode scaling, coalesced).
// ---------------------------------------------------------------------------
// Lane-interleaved rows (t1_lane.h) through buffer instructions: the group's
// region is one buffer resource (wave-uniform, SGPRs) and a row access is a
// 32-bit lane offset, so the decoder keeps one offset VGPR per row index
// instead of a 64-bit pointer per state array.
struct LRef {
    __amdgpu_buffer_rsrc_t r;
    uint32_t so, vo;
    __device__ operator uint64_t() const {
        const auto v = __builtin_amdgcn_raw_buffer_load_b64(r, vo, so, 0);
        return (uint64_t)v[0] | ((uint64_t)v[1] << 32);
    }
    __device__ const LRef &operator=(uint64_t v) const {
        const __attribute__((ext_vector_type(2))) uint32_t p = {(uint32_t)v, (uint32_t)(v >> 32)};
        __builtin_amdgcn_raw_buffer_store_b64(p, r, vo, so, 0);
        return *this;
    }
};
// so: the field's byte offset (scalar); vo: the lane's byte offset + rows
struct LRow {
    __amdgpu_buffer_rsrc_t r;
    uint32_t so, vo;
    __device__ LRef operator[](uint32_t y) const { return LRef{r, so, vo + y * 512u}; }
    __device__ LRow operator+(uint32_t n) const { return LRow{r, so, vo + n * 512u}; }
};
// the buffer resource of one 64-block group of lane-interleaved rows
__device__ __forceinline__ __amdgpu_buffer_rsrc_t group_rsrc(void *base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(base, 0, (int)bytes, 0x00020000);
}
template <int LANES>
__device__ __forceinline__ void t1_tables_init(uint8_t *zc, uint8_t *sc, uint32_t *mq) {
    for (uint32_t k = threadIdx.x; k < 2048; k += LANES) zc[k] = zc_lut_entry(k >> 9, k & 511);
    for (uint32_t k = threadIdx.x; k < 256; k += LANES) sc[k] = sc_lut_entry(k);
    for (uint32_t k = threadIdx.x; k < 47; k += LANES) mq[k] = c_mq_tab[k];
    __syncthreads();
}

// v_writelane_b32: lane `lane` of `old` replaced by the wave-uniform v.  A
// compiler that has the builtin takes it; the clang of ROCm 7.2.0 (AMD clang
// 22.0.0git, roc-7.2.0) has none, and there the declaration below binds the
// LLVM intrinsic by its name (checked on that version: one v_writelane_b32 per
// call, the hazard wait states placed by the compiler).
#if __has_builtin(__builtin_amdgcn_writelane)
__device__ __forceinline__ uint32_t wave_writelane(uint32_t v, uint32_t lane, uint32_t old) {
    return (uint32_t)__builtin_amdgcn_writelane((int)v, (int)lane, (int)old);
}
#else
extern "C" __device__ uint32_t wave_writelane(uint32_t v, uint32_t lane, uint32_t old) __asm("llvm.amdgcn.writelane.i32");
#endif

// One wavefront per block, lane = row.  Workgroup b runs on XCD b % 8 (the
// dispatcher deals workgroups round-robin), so the 64 blocks of group g are
// given to workgroups of one XCD, back to back: their row words, 8 bytes per
// lane at a 512-byte stride (the group layout, t1_lane.h EncScratch), meet as
// whole lines in that XCD's L2.
__global__ __launch_bounds__(64) void k_t1_prep(const EncBlock *__restrict__ blocks, uint32_t n, uint32_t maxdepth,
                                                const int32_t *__restrict__ coef, uint8_t *__restrict__ scr,
                                                EncResult *__restrict__ res) {
    const uint32_t wg = blockIdx.x, k = wg >> 3;
    const uint32_t i = (((k >> 6) << 3) | (wg & 7)) * 64 + (k & 63), x = threadIdx.x;
    if (i >= n) return;
    const EncBlock b = blocks[i];
    const int32_t *src = coef + b.coef_off;
    uint32_t m[64];
    uint32_t neg_lo = 0, neg_hi = 0;
    uint32_t orv = 0;
#pragma unroll
    for (int y = 0; y < 64; ++y) {
        uint32_t mv = 0, ng = 0;
        if ((uint32_t)y < b.h && x < b.w) mv = quant_mag(src[(size_t)y * b.stride + x], b.qmfbid, b.inv_step, &ng);
        m[y] = mv;
        orv |= mv;
        const uint64_t bal = __ballot(ng);
        // lane y keeps row y's ballot (a wave-uniform pair of words)
        neg_lo = wave_writelane((uint32_t)bal, y, neg_lo);
        neg_hi = wave_writelane((uint32_t)(bal >> 32), y, neg_hi);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) orv |= __shfl_xor(orv, off);
    uint32_t numbps = 0;
    if (orv) {
        uint32_t t = 32u - (uint32_t)__clz(orv);
        numbps = t <= 6 ? 0 : t - 6;
    }
    const EncScratch E = enc_scratch(scr, n, maxdepth);
    uint64_t *G = E.group(i >> 6) + (i & 63);  // row R of this block: G[R * 64]
    G[(T1E_NEG + x + 1) * 64] = x < b.h ? (uint64_t)neg_hi << 32 | neg_lo : 0;
    if (x == 0) G[T1E_NEG * 64] = 0;
    if (x == 63) G[(T1E_NEG + 65) * 64] = 0;
    const uint32_t nd = numbps < maxdepth ? numbps : maxdepth;  // numbps > maxdepth: refused (res.pad)
    // the top plane's bit (bit numbps + 5, the highest set in the block) to
    // bit 31: each plane is then the ballot of the sign bits, and one shift
    // per (row, plane) moves the next plane up
    if (nd) {
        const uint32_t up = (uint32_t)__clz(orv);
#pragma unroll
        for (int y = 0; y < 64; ++y) m[y] <<= up;
    }
    uint64_t acc = 0;  // significance before plane p = OR of the planes above
    for (uint32_t d = 0; d < nd; ++d) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int y = 0; y < 64; ++y) {
            const uint64_t bal = __ballot((int32_t)m[y] < 0);
            m[y] <<= 1;
            lo = wave_writelane((uint32_t)bal, y, lo);
            hi = wave_writelane((uint32_t)(bal >> 32), y, hi);
        }
        const uint64_t mine = (uint64_t)hi << 32 | lo;
        if (x < b.h) {
            G[(t1e_depth_row(d) + T1E_BITS + x) * 64] = mine;
            G[(t1e_depth_row(d) + T1E_ABOVE + x) * 64] = acc;
        }
        acc |= mine;
    }
    if (x == 0) {
        res[i].numbps = numbps;
        res[i].pad = 0;
    }
}

// Context modelling, one lane per (block, bit-plane): lanes are laid out
// depth-major (depth = numbps-1-p) so a wavefront holds the same depth of the
// 64 blocks of a group -- similar statistics, little divergence -- and, with
// the group-interleaved rows of t1_lane.h EncScratch, every row access of the
// wavefront is one 512-byte run.  Per-block rows (round 4) had each lane read
// its own 8-byte rows from 64 different lines, evicted between stripes: 3.3-3.7
// GB read per 8K 9/7 frame; interleaved 1.2-1.3 GB (profiles/r05/
// t1_model_interleave.txt), the post-SPP / visited rows moved from the symbol
// slots into the group rows with them.
__device__ __forceinline__ uint64_t sym_block_off(const uint64_t *sym_off, uint32_t i, uint32_t *cap) {
    if (!sym_off) {
        *cap = 32;
        return (uint64_t)i * 32 * sym_slot_bytes(64, 64);
    }
    return sym_off[i];
}

template <bool COND>
__global__ __launch_bounds__(64) void k_t1_model(
    const EncBlock *__restrict__ blocks, uint32_t n, uint32_t maxdepth, uint8_t *__restrict__ scr,
    uint8_t *__restrict__ sym, const uint64_t *__restrict__ sym_off, EncResult *__restrict__ res, uint32_t cblksty) {
    __shared__ __attribute__((aligned(8))) uint32_t s_ctab[512];  // compact_sel {lo, hi} of every presence byte
    __shared__ uint32_t s_ring[32 * 64];  // SymOut: 32 words per lane, word j at (j % 32) * 64 + lane
    for (uint32_t k = threadIdx.x; k < 256; k += 64) compact_sel(k, &s_ctab[2 * k], &s_ctab[2 * k + 1]);
    __syncthreads();
    // wavefront = (group, depth): lane = the group's block
    const uint32_t n64 = t1_scratch_records(n), w0 = blockIdx.x * 64;
    const uint32_t g0 = w0 % n64, d = w0 / n64, i = g0 + threadIdx.x;
    if (d >= maxdepth || i >= n) return;
    const uint32_t numbps = res[i].numbps;
    if (d >= numbps) return;
    const EncBlock b = blocks[i];
    const uint32_t slot = sym_slot_bytes(b.w, b.h);
    uint32_t cap = 0;
    const uint64_t off = sym_block_off(sym_off, i, &cap);
    if (sym_off) cap = (uint32_t)((sym_off[i + 1] - off) / slot);
    if (numbps > cap) {
        if (d == 0) res[i].pad = 1;  // numbps above the band's bound: reported by the host
        return;
    }
    const uint32_t p = numbps - 1 - d;
    const EncScratch E = enc_scratch(scr, n, maxdepth);
    const __amdgpu_buffer_rsrc_t gr = group_rsrc(E.group(g0 >> 6), 64 * E.rec_rows * 8);
    const uint32_t lo = threadIdx.x * 8, dr = t1e_depth_row(d);
    const LRow bits{gr, (dr + T1E_BITS) * 512, lo}, above{gr, (dr + T1E_ABOVE) * 512, lo};
    const LRow ref{gr, (d ? dr - T1E_DEPTH_ROWS + T1E_ABOVE : 0) * 512, lo}, negr{gr, T1E_NEG * 512, lo};
    const LRow tmp{gr, (dr + T1E_POST) * 512, lo};
    uint8_t *base = sym + off + (uint64_t)p * slot;
    t1_model_plane<LRow, LRow, COND>(b.w, b.h, b.orient, bits, above, ref, d > 0, negr, tmp, nullptr, (uint32_t *)base,
                   E.cnt + (size_t)i * 128 + p * 4, cblksty, t1_pass_raw(cblksty, (int32_t)p, 0, numbps),
                   s_ring + threadIdx.x, s_ctab);
}

constexpr uint32_t MQ_CX_STRIDE = 21;  // LDS words per lane for the MQ encoder's context words

// MQ coding, one lane per block (lane j codes block perm[j], or j).  WAVES
// wavefronts per workgroup share the state table and the read-ahead slack
// (CXS: context words per lane).
template <int LANES, int MINW = 1, bool LAZY = false, int WAVES = 1, uint32_t CXS = MQ_CX_STRIDE>
__global__ __launch_bounds__(LANES * WAVES, MINW) void k_t1_mq(const EncBlock *__restrict__ blocks, uint32_t n,
                                                 const uint32_t *__restrict__ cnt, const uint8_t *__restrict__ sym,
                                                 const uint64_t *__restrict__ sym_off, uint8_t *__restrict__ out,
                                                 EncResult *__restrict__ res, const uint32_t *__restrict__ perm,
                                                 uint32_t cblksty, uint32_t bpw) {
    __shared__ uint32_t s_mq[48];
    // 19 context words per lane at an odd stride (no bank conflicts).  The
    // read-ahead of the symbol after a pass's last one may index up to 31
    // (its value is never used): the next lane's slots, or for the last lane
    // the tail slack, keep it inside the array.
    __shared__ uint32_t s_cx[WAVES * LANES * CXS + 32];
    for (uint32_t k = threadIdx.x; k < 47; k += LANES * WAVES) s_mq[k] = c_mq_tab[k];
    __syncthreads();
    const uint32_t lane = threadIdx.x % LANES;
    if (lane >= bpw) return;  // bpw blocks per wavefront (t1_blocks_per_wave)
    const uint32_t j = (blockIdx.x * WAVES + threadIdx.x / LANES) * bpw + lane;
    if (j >= n) return;
    const uint32_t i = perm ? perm[j] : j;
    const EncBlock b = blocks[i];
    EncResult &r = res[i];
    if (r.pad) return;
    uint32_t cap;
    const uint64_t off = sym_block_off(sym_off, i, &cap);
    uint32_t len;
    uint32_t np = t1_mq_block<LAZY>(r.numbps, (const uint32_t *)(sym + off), sym_slot_bytes(b.w, b.h) / 4, cnt + (size_t)i * 128, s_mq,
                              s_cx + threadIdx.x * CXS, (uint32_t *)(out + b.out_off), r.rate, &len, cblksty);
    r.numpasses = np;
    r.len = len;
    uint32_t nsym = 0;
    const uint32_t *c = cnt + (size_t)i * 128;
    for (uint32_t q = 0; q < r.numbps && q < 32; ++q) nsym += c[q * 4] + c[q * 4 + 1] + c[q * 4 + 2];
    r.nsym = nsym;
}

// Work order for k_t1_mq (the decoder's host-side order, on the device: the
// encoder's work per block is only known after k_t1_model).  A counting sort
// of the blocks by their symbol count, heaviest first, in MQ_ORDER_BUCKETS
// log-spaced buckets (8 per octave): per block its bucket, a histogram with
// vector atomics, an exclusive scan in one workgroup, then a scatter.  The
// order inside a bucket follows the atomics (it varies from run to run);
// every block's output is its own, so the codestream does not.
constexpr uint32_t MQ_ORDER_BUCKETS = 256;
__device__ __forceinline__ uint32_t mq_work_bucket(const uint32_t *c, uint32_t numbps) {
    uint32_t w = 0;
    for (uint32_t q = 0; q < numbps && q < 32; ++q) w += c[q * 4] + c[q * 4 + 1] + c[q * 4 + 2];
    w += 1;
    const uint32_t o = 31u - (uint32_t)__builtin_clz(w);            // octave
    const uint32_t f = o >= 3 ? (w >> (o - 3)) & 7u : (w << (3 - o)) & 7u;  // 3 bits below the top one
    return (MQ_ORDER_BUCKETS - 1) - min((o << 3) | f, MQ_ORDER_BUCKETS - 1);  // heaviest first
}
__global__ __launch_bounds__(256) void k_mq_order_hist(const uint32_t *__restrict__ cnt,
                                                      const EncResult *__restrict__ res, uint32_t n,
                                                      uint32_t *__restrict__ key, uint32_t *__restrict__ hist) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = mq_work_bucket(cnt + (size_t)i * 128, res[i].numbps);
    key[i] = k;
    atomicAdd(&hist[k], 1u);
}
__global__ __launch_bounds__(MQ_ORDER_BUCKETS) void k_mq_order_scan(uint32_t *__restrict__ hist) {
    __shared__ uint32_t s[MQ_ORDER_BUCKETS];
    const uint32_t t = threadIdx.x;
    s[t] = hist[t];
    __syncthreads();
    for (uint32_t d = 1; d < MQ_ORDER_BUCKETS; d <<= 1) {  // inclusive Hillis-Steele scan
        const uint32_t v = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    hist[t] = s[t] - hist[t];  // exclusive: the bucket's first slot
}
__global__ __launch_bounds__(256) void k_mq_order_scatter(const uint32_t *__restrict__ key, uint32_t n,
                                                         uint32_t *__restrict__ next, uint32_t *__restrict__ perm) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    perm[atomicAdd(&next[key[i]], 1u)] = i;
}

// Per-pass distortion sums (the nmsedec of t1_enc_sigpass / refpass /
// clnpass, t1.cpp:197-338, 443-555, 639-782 with t1_getnmsedec_sig/_ref
// :155-166): one wavefront per block, lane = column.  A sample contributes
// to the plane of its most significant bit (significance: to the SPP when
// the modelling kernel found it significant during that plane's SPP, else
// to the cleanup pass) and to every lower plane's refinement pass.  The
// SPP membership comes from the post-SPP significance rows k_t1_model left
// behind each plane's symbol stream.
__global__ __launch_bounds__(64) void k_t1_dist(const EncBlock *__restrict__ blocks, uint32_t n, uint32_t maxdepth,
                                                const int32_t *__restrict__ coef, const uint8_t *__restrict__ scr,
                                                EncResult *__restrict__ res, NmseLut lutv) {
    __shared__ NmseLut lut;
    {
        const int16_t *src = &lutv.sig[0];
        int16_t *dst = &lut.sig[0];
        for (uint32_t k = threadIdx.x; k < 512; k += 64) dst[k] = src[k];
    }
    __syncthreads();
    const uint32_t i = blockIdx.x, x = threadIdx.x;
    const EncBlock b = blocks[i];
    EncResult &r = res[i];
    const uint32_t numbps = r.numbps;
    if (numbps == 0 || r.pad) return;
    const int32_t *src = coef + b.coef_off;
    uint32_t m[64];
#pragma unroll
    for (int y = 0; y < 64; ++y) {
        uint32_t ng;
        m[y] = ((uint32_t)y < b.h && x < b.w) ? quant_mag(src[(size_t)y * b.stride + x], b.qmfbid, b.inv_step, &ng) : 0;
    }
    const EncScratch E = enc_scratch(const_cast<uint8_t *>(scr), n, maxdepth);
    const uint64_t *G = E.group(i >> 6) + (i & 63);
    for (int32_t p = (int32_t)numbps - 1; p >= 0; --p) {
        // the block's post-SPP significance rows of plane p (row y at post[y * 64])
        const uint64_t *post = G + (size_t)(t1e_depth_row(numbps - 1 - (uint32_t)p) + T1E_POST) * 64;
        int32_t a0 = 0, a1 = 0, a2 = 0;
#pragma unroll
        for (int y = 0; y < 64; ++y) {
            const uint32_t mag = (uint32_t)y < b.h ? m[y] : 0u;  // no break: m stays in registers
            const uint32_t win = p > 0 ? (mag >> p) & 127u : mag & 127u;
            if ((mag >> (p + 6)) == 1u) {
                const int32_t v = p > 0 ? lut.sig[win] : lut.sig0[win];
                if ((post[(size_t)y * 64] >> x) & 1u) a0 += v; else a2 += v;
            } else if (mag >> (p + 7)) {
                a1 += p > 0 ? lut.ref[win] : lut.ref0[win];
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            a0 += __shfl_xor(a0, o);
            a1 += __shfl_xor(a1, o);
            a2 += __shfl_xor(a2, o);
        }
        if (x == 0) {
            if (p == (int32_t)numbps - 1) {
                r.nmsedec[0] = a2;
            } else {
                const uint32_t base = 1 + 3 * (numbps - 2 - (uint32_t)p);
                r.nmsedec[base] = a0;
                r.nmsedec[base + 1] = a1;
                r.nmsedec[base + 2] = a2;
            }
        }
    }
}

// T1 decoder (t1_flat.h t1_decode_v5).  Pass 1, lane per block: remove the MQ
// byte stuffing into a plain bit stream + carry events (region of block i at
// ubuf + i * fixed_words words, or at blocks[i].pad * 16 bytes when
// fixed_words == 0: header {nwords, ncarry}, words, carries).  Pass 2, lane
// per block: the pass / stripe / column walk over the unstuffed stream.
__device__ __forceinline__ size_t ub_region(const DecBlock &b, uint32_t i, uint32_t fixed_words) {
    return fixed_words ? (size_t)i * fixed_words : (size_t)b.pad * 4;
}

// unstuff one segment (len bytes at data + data_off) into region: header
// {nwords, ncarry}, words, carries
__device__ __forceinline__ void unstuff_segment(const uint8_t *__restrict__ data, uint64_t data_off, uint32_t len,
                                                uint32_t *__restrict__ region) {
    uint32_t *words = region + 4, *carries = words + unstuff_word_cap(len);
    const uintptr_t pa = (uintptr_t)(data + data_off);
    const uint4 *src = (const uint4 *)(pa & ~(uintptr_t)15);
    const uint32_t skip = (uint32_t)(pa & 15), end = skip + len;
    const uint32_t nch = (end + 15) >> 4;
    Unstuff u;
    uint32_t nw = 0, nc = 0;
    uint4 nxt = nch ? src[0] : uint4{0, 0, 0, 0};
    for (uint32_t ch = 0; ch < nch; ++ch) {
        const uint4 cur = nxt;
        if (ch + 1 < nch) nxt = src[ch + 1];
        const uint32_t wv4[4] = {cur.x, cur.y, cur.z, cur.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t pos = ch * 16 + j;
            if (pos < skip || pos >= end) continue;
            uint32_t wv, cv;
            if (u.push((wv4[j >> 2] >> (8 * (j & 3))) & 0xffu, &wv, &cv)) words[nw++] = wv;
            if (cv != 0xffffffffu) carries[nc++] = cv;
        }
    }
    words[nw++] = u.tail();
    do { words[nw++] = 0xffffffffu; } while (nw & 3);
    for (int k = 0; k < 8; ++k) words[nw++] = 0xffffffffu;
    carries[nc] = 0xffffffffu;
    region[0] = nw;
    region[1] = nc;
}

// segs / seg_first (codestream decode): block i's segments are
// segs[seg_first[i] .. seg_first[i+1]); null: one segment per block at
// blocks[i].data_off (the stage entry point)
__global__ __launch_bounds__(64) void k_t1_unstuff(const DecBlock *__restrict__ blocks, uint32_t n,
                                                   const uint8_t *__restrict__ data, uint32_t *__restrict__ ubuf,
                                                   uint32_t fixed_words, const DecSeg *__restrict__ segs,
                                                   const uint32_t *__restrict__ seg_first) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const DecBlock b = blocks[i];
    if (b.len == 0 || b.numpasses == 0 || b.numbps == 0 || b.numbps > T1_MAX_DEC_BPS) return;
    if (segs) {
        for (uint32_t q = seg_first[i]; q < seg_first[i + 1]; ++q) {
            const DecSeg sg = segs[q];
            unstuff_segment(data, sg.data_off, sg.len, ubuf + (size_t)sg.ub_off * 4);
        }
        return;
    }
    unstuff_segment(data, b.data_off, b.len, ubuf + ub_region(b, i, fixed_words));
}

// The same pre-pass with one wavefront per code-block segment: 64 bytes per
// step, one per lane.  A byte's bit count (7 after a 0xFF, else 8) and its
// bit position in the output stream come from a wave prefix sum, its bits are
// ORed into the step's words in LDS (a byte may straddle two words), the
// completed words leave as one coalesced store, the partial last one stays
// for the next step; a marker (0xFF then > 0x8F) ends the stream at the first
// lane holding one, and carry events are compacted by ballot in stream
// order.  Output identical to unstuff_segment's.  The lane-per-block pass runs
// 64 blocks' serial byte loops per wavefront -- ~390 wavefronts for a whole
// 8K frame, a long dependent chain per lane: the shorter chain for a call
// alone on the GPU, the fewer instructions for a batch (launch_t1_decode).
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t lane, uint32_t *tot) {
    uint32_t x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t y = __shfl_up(x, d, 64);
        x += lane >= (uint32_t)d ? y : 0u;
    }
    *tot = __shfl(x, 63, 64);
    return x - v;
}

__device__ void unstuff_segment_wave(const uint8_t *__restrict__ data, uint64_t data_off, uint32_t len,
                                     uint32_t *__restrict__ region, uint32_t *wbuf, uint32_t lane) {
    uint32_t *words = region + 4, *carries = words + unstuff_word_cap(len);
    uint32_t bitpos = 0, nc = 0;  // bits emitted, carry events written
    bool pff_in = false;          // the byte before this step's first one is 0xFF
    if (lane < 20) wbuf[lane] = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (uint32_t base = 0; base < len; base += 64) {
        const uint32_t j = base + lane;
        const bool inb = j < len;
        const uint32_t b = inb ? (uint32_t)data[data_off + j] : 0u;
        const uint32_t prev = __shfl_up(b, 1, 64);
        const bool pff = lane ? prev == 0xffu : pff_in;
        const uint64_t mk = __ballot(inb && pff && b > 0x8fu);  // markers: the stream ends at the first
        const uint32_t first = mk ? (uint32_t)__builtin_ctzll(mk) : 64u;
        const bool valid = inb && lane < first;
        const uint32_t nb = valid ? (pff ? 7u : 8u) : 0u;
        uint32_t tot;
        const uint32_t o = bitpos + wave_excl_scan(nb, lane, &tot);
        // carry event: a stuffed byte's top bit (see Unstuff)
        const bool ev = valid && pff && (b & 0x80u);
        const uint64_t em = __ballot(ev);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(em >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)em, 0u));
        if (ev) carries[nc + rank] = o - 1 + 17;
        nc += (uint32_t)__builtin_popcountll(em);
        // the byte's bits at stream bits [o, o + nb), MSB first; word index relative to this step's first
        if (nb) {
            const uint32_t v = b & (pff ? 0x7fu : 0xffu);
            const uint32_t k = (o >> 5) - (bitpos >> 5), p = o & 31u, e = p + nb;
            if (e <= 32) {
                atomicOr(&wbuf[k], v << (32 - e));
            } else {
                atomicOr(&wbuf[k], v >> (e - 32));
                atomicOr(&wbuf[k + 1], v << (64 - e));
            }
        }
        // one wavefront's LDS operations complete in order; the fence keeps the
        // compiler from moving the reads above the ORs (no workgroup barrier:
        // the other wavefronts of the workgroup work on other blocks)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const uint32_t end = bitpos + tot, done = (end >> 5) - (bitpos >> 5);  // completed words
        uint32_t w = lane < 20 ? wbuf[lane] : 0u;
        if (lane < done) words[(bitpos >> 5) + lane] = w;
        // the partial word moves to slot 0, the rest is cleared
        const uint32_t carry_w = __shfl(w, (int)done, 64);
        if (lane < 20) wbuf[lane] = lane == 0 ? carry_w : 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        bitpos = end;
        pff_in = __shfl(b, 63, 64) == 0xffu;
        if (mk) break;
    }
    // tail (Unstuff::tail): the pending bits, then 1-bits; a word of 1-bits
    // when none is pending; then 1-bit words to a multiple of 4 and 8 more
    const uint32_t nw0 = bitpos >> 5, pend = bitpos & 31u;
    const uint32_t w0 = __shfl(lane < 20 ? wbuf[lane] : 0u, 0, 64);
    const uint32_t tailw = pend ? (w0 | ((1u << (32 - pend)) - 1u)) : 0xffffffffu;
    uint32_t nw = nw0 + 1;
    nw += (4 - (nw & 3)) & 3;
    if ((nw - nw0 - 1) == 0) nw += 4;  // the serial pass writes at least one 1-bit word after the tail
    nw += 8;
    for (uint32_t q = lane; nw0 + q < nw; q += 64) words[nw0 + q] = q == 0 ? tailw : 0xffffffffu;
    if (lane == 0) {
        carries[nc] = 0xffffffffu;
        region[0] = nw;
        region[1] = nc;
    }
}

__global__ __launch_bounds__(256) void k_t1_unstuff_w(const DecBlock *__restrict__ blocks, uint32_t n,
                                                     const uint8_t *__restrict__ data, uint32_t *__restrict__ ubuf,
                                                     uint32_t fixed_words, const DecSeg *__restrict__ segs,
                                                     const uint32_t *__restrict__ seg_first) {
    __shared__ uint32_t s_w[4][20];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t i = blockIdx.x * 4 + wv;
    if (i >= n) return;
    const DecBlock b = blocks[i];
    if (b.len == 0 || b.numpasses == 0 || b.numbps == 0 || b.numbps > T1_MAX_DEC_BPS) return;
    if (segs) {
        for (uint32_t q = seg_first[i]; q < seg_first[i + 1]; ++q) {
            const DecSeg sg = segs[q];
            unstuff_segment_wave(data, sg.data_off, sg.len, ubuf + (size_t)sg.ub_off * 4, s_w[wv], lane);
        }
        return;
    }
    unstuff_segment_wave(data, b.data_off, b.len, ubuf + ub_region(b, i, fixed_words), s_w[wv], lane);
}

struct LState {
    LRow sig, neg, vis, ref;
};

// Decoder workgroups: DEC_WAVES wavefronts share one copy of the LUTs in LDS,
// and the kernel is held to 128 VGPRs (a few spills at pass boundaries), so 4
// wavefronts fit per SIMD by both registers and LDS (38 KB per workgroup: the
// LUTs, 19 context words per lane -- odd, so the lanes spread over the banks --
// and the bit readers' word rings).  Against one wavefront per workgroup at 144
// VGPRs (3 per SIMD): 8K batch 3264-3280 -> 3507-3508 Mpixels/s, lone decode
// T1 31.7-31.9 -> 30.9-31.3 ms (profiles/r05/t1_dec_wg_ab.txt).  (Round 3's
// 128-VGPR build with single-wavefront workgroups had measured no gain: LDS
// then still held it near 3 per SIMD.)
constexpr int DEC_WAVES = 4;
constexpr uint32_t DEC_CX_STRIDE = 19;

template <int LANES, bool LAZY, int WAVES, int WPE>
__global__ __launch_bounds__(LANES * WAVES) __attribute__((amdgpu_waves_per_eu(WPE))) void k_t1_decode_ub(const DecBlock *__restrict__ blocks, uint32_t n,
                                                        const uint32_t *__restrict__ ubuf, uint32_t fixed_words,
                                                        T1Scratch *__restrict__ scr, const DecSeg *__restrict__ segs,
                                                        const uint32_t *__restrict__ seg_first, uint32_t sty,
                                                        const uint8_t *__restrict__ roi, uint32_t bpw) {
    __shared__ uint8_t s_zc[2048];
    __shared__ uint8_t s_sc[256];
    __shared__ uint32_t s_mq[MQ_DEC_WORDS + 2];  // decoder successor table (t1_lane.h mq_dec_table_entry)
    __shared__ uint32_t s_cx[WAVES * LANES * DEC_CX_STRIDE];
    __shared__ uint32_t s_ring[WAVES * LANES * FB_RING];  // bit readers' word rings (t1_flat.h FlatBits), slot stride 64
    static_assert(LANES == 64, "the word rings interleave 64 lanes");
    for (uint32_t k = threadIdx.x; k < 2048; k += LANES * WAVES) s_zc[k] = zc_lut_entry(k >> 9, k & 511);
    for (uint32_t k = threadIdx.x; k < 256; k += LANES * WAVES) s_sc[k] = sc_win_entry(k);
    for (uint32_t k = threadIdx.x; k < MQ_DEC_WORDS; k += LANES * WAVES) s_mq[k] = mq_dec_table_entry(c_mq_tab, k);
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane >= bpw) return;  // bpw blocks per wavefront (t1_blocks_per_wave)
    const uint32_t gw = blockIdx.x * WAVES + wv;  // the wavefront's index in the grid
    const uint32_t i = gw * bpw + lane;
    if (i >= n) return;
    const DecBlock b = blocks[i];
    if (b.len == 0 || b.numpasses == 0 || b.numbps == 0 || b.numbps > T1_MAX_DEC_BPS) return;
    const DecTables T{s_zc + b.orient * 512, s_sc, s_mq};
    // lane-interleaved state and bit-plane rows of this block (t1_lane.h T1Group)
    // bpw is a power of two <= 64, so the wavefront's blocks share one group:
    // the group (and the buffer resource) stays wave-uniform, in SGPRs
    const uint32_t grp = __builtin_amdgcn_readfirstlane((gw * bpw) >> 6);
    const __amdgpu_buffer_rsrc_t gr = __builtin_amdgcn_make_buffer_rsrc(
        t1_group_base(scr, grp, sizeof(T1Scratch)), 0, (int)(64 * sizeof(T1Scratch)), 0x00020000);
    const uint32_t lo = (i & 63) * 8;
    LState st{LRow{gr, T1R_SIG * 512, lo}, LRow{gr, T1R_NEG * 512, lo}, LRow{gr, T1R_VIS * 512, lo},
              LRow{gr, T1R_REF * 512, lo}};
    const LRow pa{gr, T1R_PA * 512, lo}, pb{gr, T1R_PB * 512, lo};
    uint32_t *const ring = s_ring + wv * (LANES * FB_RING) + lane;
    uint32_t *cxw = s_cx + threadIdx.x * DEC_CX_STRIDE;
    if (segs) {
        const uint32_t q0 = seg_first[i], nseg = seg_first[i + 1] - q0;
        const DecSeg s0 = segs[q0];
        const uint32_t *region = ubuf + (size_t)s0.ub_off * 4;
        for (uint32_t y = 0; y < b.h + 2; ++y) { st.sig[y] = 0; st.neg[y] = 0; st.vis[y] = 0; st.ref[y] = 0; }
        mq_reset_words_dec(cxw, T.mq);
        BitDecT<LAZY> d;
        d.set_ring(ring, 6);
        d.init(region + 4, region[0], region + 4 + unstuff_word_cap(s0.len));
        SegCursor cur{segs + q0, ubuf, nseg, 0, s0.npasses};
        t1_decode_passes(d, b.numpasses, b.numbps, b.w, b.h, st, T, cxw, pa, pb, sty, cur, roi ? roi[i] : 0u);
        return;
    }
    const uint32_t *region = ubuf + ub_region(b, i, fixed_words);
    t1_decode_v5(region + 4, region[0], region + 4 + unstuff_word_cap(b.len), b.numpasses, b.numbps, b.w, b.h, st, T,
                 cxw, pa, pb, ring, 6);
}

// Rebuild of the decoded values from the lane-interleaved bit-plane rows, on
// the scalar side.  A wavefront takes an octet -- 8 adjacent blocks of a
// group, 64 bytes of every plane row (row R of block b of a group is word
// R * 64 + b) -- for RB_ROWS rows; lane x forms the coefficients of column x.
// Every 64-bit row mask is wave-uniform: one 64-byte scalar load brings the
// octet's words of a (plane, row), the magnitude bit-plane
//   M_q = (S_q & ~above) | (R_q & above),   above = S_{q+1} | S_{q+2} | ..
// (S sigafter, R refbit: the first significant plane's bit is 1, the planes
// under it carry their refinement bits) is formed per block in SGPRs, and the
// lane takes its bit with a select on that mask and a shift-or: 2 VALU per
// (block, plane), no LDS, no barrier.  The value is t1_rebuild's (t1_lane.h):
// with m the magnitude bits at their planes, 2 * m + min(m, 1 << qlow).
// The blocks of an octet differ in their planes and shapes: a plane outside a
// block's [low, top] (sigafter) or [qlow, top - 1] (refbit) is replaced by 0
// by a scalar select on the block's plane sets, and the rows read are those
// of the union over the octet's blocks that have the row -- what the decoder
// wrote.  A 64-byte load also brings the words of the octet's blocks that
// lack that plane or row and of the lanes past the last block: words the
// decoder may not have written (they lie inside the scratch, whose groups are
// whole -- t1_scratch_records), read and then dropped -- the plane-set select
// replaces them by 0, and a block without the row is skipped before its
// accumulator is used.  The refbit words R likewise keep the row's last
// loaded plane (0 at first) where no block has a refinement row: every
// rf[b] select is then 0.
// Then T1Part1::postDecode scaling (5/3: v/2, 9/7: float(v) * step).
// roi (null: none): per-block ROI up-shift -- T1Part1::post_decode
// (T1Part1.cpp:230-250) shifts magnitudes >= 2^roishift down by roishift (and
// zeroes the block for a shift >= 31) before the scaling.
constexpr uint32_t RB_ROWS = 8, RB_WAVES = 4;
typedef uint64_t rb_octet __attribute__((ext_vector_type(8)));
// one plane of the octet; ALL: every block has the plane in both sets
template <bool ALL>
__device__ __forceinline__ void rb_plane(const rb_octet &S, const rb_octet &R, const uint32_t (&in)[8],
                                         const uint32_t (&rf)[8], uint32_t q, uint32_t sh, uint64_t (&above)[8],
                                         uint32_t (&acc)[8]) {
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
        const uint64_t s = ALL || ((in[b] >> q) & 1u) ? S[b] : 0, r = ALL || ((rf[b] >> q) & 1u) ? R[b] : 0;
        const uint64_t m = (s & ~above[b]) | (r & above[b]);
        above[b] |= s;
        acc[b] = (acc[b] << sh) | (__builtin_amdgcn_inverse_ballot_w64(m) ? 1u : 0u);
    }
}
__global__ __launch_bounds__(64 * RB_WAVES) void k_t1_rebuild(const DecBlock *__restrict__ blocks, uint32_t n,
                                                              const T1Scratch *__restrict__ scr,
                                                              int32_t *__restrict__ tiles,
                                                              const uint8_t *__restrict__ roi) {
    const uint32_t l = threadIdx.x & 63;
    const uint32_t i0 = (blockIdx.x * RB_WAVES + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)) * 8;
    if (i0 >= n) return;
    const uint32_t nb = n - i0 < 8 ? n - i0 : 8;
    const uint32_t y0 = blockIdx.y * RB_ROWS;
    // lane b < nb holds block b's parameters: the plane sets of its sigafter
    // and refbit rows stay in SGPRs, what forms and stores the value is
    // read from the lane once per row
    DecBlock mb{};
    uint32_t in_l = 0, rf_l = 0, pk = 0;
    if (l < nb) {
        mb = blocks[i0 + l];
        const DecodedPlanes dp = decoded_planes(mb.len && mb.numbps <= T1_MAX_DEC_BPS ? mb.numpasses : 0, mb.numbps);
        if (dp.top >= 0) {
            in_l = ((2u << dp.top) - 1) & ~((1u << dp.low) - 1);
            if (dp.qlow < 32) rf_l = ((1u << dp.top) - 1) & ~((1u << dp.qlow) - 1);
        }
        // the half-LSB term's bound 1 << qlow (qlow = 32: none, m < 2^30), the width, 9/7, the ROI shift
        pk = (dp.qlow < 30 ? (uint32_t)dp.qlow : 30u) | mb.w << 8 | (mb.irrev ? 1u << 16 : 0u) |
             (roi ? (uint32_t)roi[i0 + l] << 24 : 0u);
    }
    uint32_t in[8], rf[8], bh[8], hmax = 0, hmin = 64;
    // over the octet's blocks: the planes some block has, and those all of them have in both sets
    uint32_t uin0 = 0, urf0 = 0, all0 = ~0u;
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
        in[b] = __builtin_amdgcn_readlane(in_l, b);
        rf[b] = __builtin_amdgcn_readlane(rf_l, b);
        bh[b] = __builtin_amdgcn_readlane(mb.h, b);
        hmax = bh[b] > hmax ? bh[b] : hmax;
        if (bh[b]) {
            hmin = bh[b] < hmin ? bh[b] : hmin;
            uin0 |= in[b];
            urf0 |= rf[b];
            all0 &= in[b] & rf[b];
        }
    }
    const uint64_t *gb = t1_group_base(const_cast<T1Scratch *>(scr), i0 >> 6, sizeof(T1Scratch)) + (i0 & 56);
    const uint32_t y1 = y0 + RB_ROWS < hmax ? y0 + RB_ROWS : hmax;
    for (uint32_t y = y0; y < y1; ++y) {
        // the same over the blocks that have this row
        uint32_t uin = uin0, urf = urf0, all = all0;
        if (y >= hmin) {
            uin = urf = 0;
            all = ~0u;
#pragma unroll
            for (uint32_t b = 0; b < 8; ++b)
                if (y < bh[b]) {
                    uin |= in[b];
                    urf |= rf[b];
                    all &= in[b] & rf[b];
                }
        }
        uint32_t acc[8];
        uint64_t above[8];
        rb_octet S, R = 0, N = 0;
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) { acc[b] = 0; above[b] = 0; }
        uint32_t ql = uin ? 31u - (uint32_t)__builtin_clz(uin) : 0;  // the last plane taken
        for (uint32_t rem = uin; rem;) {
            const uint32_t q = 31u - (uint32_t)__builtin_clz(rem), sh = ql - q;  // planes no block has are skipped
            ql = q;
            rem &= ~(1u << q);
            S = *(const rb_octet *)(gb + (size_t)(T1R_PA + q * 64 + y) * 64);
            if ((urf >> q) & 1u) R = *(const rb_octet *)(gb + (size_t)(T1R_PB + q * 64 + y) * 64);
            if ((all >> q) & 1u) rb_plane<true>(S, R, in, rf, q, sh, above, acc);
            else rb_plane<false>(S, R, in, rf, q, sh, above, acc);
        }
        if (uin) N = *(const rb_octet *)(gb + (size_t)(T1R_NEG + y + 1) * 64);
#pragma unroll
        for (uint32_t b = 0; b < 8; ++b) {
            if (y >= bh[b]) continue;  // uniform
            const uint32_t bpk = __builtin_amdgcn_readlane(pk, b);
            const uint32_t m = acc[b] << ql, hb = 1u << (bpk & 0xff), brs = bpk >> 24;
            int32_t mag = (int32_t)(2 * m + (m < hb ? m : hb));
            if (brs) mag = brs >= 31 ? 0 : (mag >= (1 << brs) ? mag >> brs : mag);
            const int32_t v = __builtin_amdgcn_inverse_ballot_w64(N[b]) ? -mag : mag;
            const float step = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mb.step), b));
            const int32_t o = (bpk >> 16) & 1u ? __float_as_int(__fmul_rn((float)v, step)) : v / 2;
            const uint32_t off_lo = __builtin_amdgcn_readlane((uint32_t)mb.dst_off, b);
            const uint32_t off_hi = __builtin_amdgcn_readlane((uint32_t)(mb.dst_off >> 32), b);
            const uint32_t stride = __builtin_amdgcn_readlane(mb.dstride, b);
            if (l < ((bpk >> 8) & 0xff)) tiles[(((uint64_t)off_hi << 32) | off_lo) + (size_t)y * stride + l] = o;
        }
    }
}

// Codestream assembly: copy each run (header bytes from the host-written blob,
// or a code-block's MQ bytes from the T1 slab) to its final offset.
__global__ void k_gather(const uint8_t *__restrict__ hdr, const uint8_t *__restrict__ slab,
                         const GatherItem *__restrict__ items, uint32_t n, uint8_t *__restrict__ dst) {
    uint32_t i = blockIdx.x;
    if (i >= n) return;
    GatherItem it = items[i];
    const uint8_t *src = (it.pad ? slab : hdr) + it.src;
    for (uint32_t k = threadIdx.x; k < it.len; k += blockDim.x) dst[it.dst + k] = src[k];
}

// ---------------------------------------------------------------------------
// launchers (host side, used by codec.cpp)
// ---------------------------------------------------------------------------
// the load mode of a source format with its flags (kernel template M: bit 0
// big-endian, bit 1 interleaved; one component's pixels are its plane); -1: a
// flag the format cannot carry
static int src_mode(int32_t fmt, uint32_t ncomp) {
    if (fmt & ~(0xff | SMP_INTERLEAVED | SMP_BIG_ENDIAN)) return -1;
    const int32_t w = fmt & 0xff;
    if ((fmt & SMP_BIG_ENDIAN) && w != SMP_U16 && w != SMP_I16) return -1;
    return ((fmt & SMP_BIG_ENDIAN) ? 1 : 0) | ((fmt & SMP_INTERLEAVED) && ncomp > 1 ? 2 : 0);
}

// f(T{}) with the sample type T of fmt (a SampleFmt without flags), then the
// error of what f launched; hipErrorInvalidValue for any other fmt
template <typename F>
static hipError_t with_sample_type(int32_t fmt, F &&f) {
    switch (fmt) {
        case SMP_I32: f(int32_t{}); break;
        case SMP_U8: f(uint8_t{}); break;
        case SMP_I8: f(int8_t{}); break;
        case SMP_U16: f(uint16_t{}); break;
        case SMP_I16: f(int16_t{}); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
// The formats with a colour conversion (sYCC / eYCC / CMYK output is unsigned)
// and with the 4:2:0 run kernel: U8 / U16 / I32.  The signed narrow formats
// have the OP = 0 and OP_PREC instantiations only.
// The float formats hold every precision and sign: colour formats too.
template <typename T>
constexpr bool colour_fmt = std::is_unsigned<T>::value || sizeof(T) == 4 || float_tag<T>;
constexpr bool colour_fmt_of(int32_t fmt) { return fmt == SMP_I32 || fmt == SMP_U8 || fmt == SMP_U16 || float_fmt(fmt); }
// with_sample_type for the float formats: the launchers with ops take them
// (OP != 0 instantiations only), every other launcher refuses them as unknown
template <typename F>
static hipError_t with_float_type(int32_t fmt, F &&f) {
    switch (fmt) {
        case SMP_F32: f(SmpF32{}); break;
        case SMP_F16: f(SmpF16{}); break;
        case SMP_BF16: f(SmpBF16{}); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
// ... and for any output format of a launcher with ops
template <typename F>
static hipError_t with_out_type(int32_t fmt, F &&f) {
    return float_fmt(fmt) ? with_float_type(fmt, f) : with_sample_type(fmt, f);
}
// a compile-time OP / flag handed to a generic lambda
template <int V>
using Const = std::integral_constant<int, V>;
// f(Const<OP>{}) with the OP the ops select (sycc_launchable holds): the
// colour conversion in the formats that have one, else the precision ops alone
template <typename T, typename F>
static void with_op(const OutOps &ops, F &&f) {
    if constexpr (colour_fmt<T>) {
        if (ops.sycc) return f(Const<OP_SYCC>{});
        if (ops.col == COL_EYCC) return f(Const<OP_EYCC>{});
        if (ops.col == COL_CMYK) return f(Const<OP_CMYK>{});
    }
    f(Const<OP_PREC>{});
}
// the (row threads, rows) grid of the kernels that own runs of 16 bytes: the
// lead run + the runs of NarrowRun<T>::N pixels along a row of tw
template <typename T>
static dim3 run_grid(uint32_t tw, uint32_t rows) {
    const uint32_t runs = (uint32_t)(((uint64_t)tw + NarrowRun<T>::N - 1) / NarrowRun<T>::N + 1);
    return dim3((runs + 255) / 256, rows);
}
// ... and of the kernels with a thread per pixel
static dim3 pixel_grid(uint32_t tw, uint32_t rows) { return dim3((tw + 255) / 256, rows); }

hipError_t launch_dcshift_mct_fwd(const SrcPlanes &src, int32_t fmt, uint32_t sstride, const PlanePtrs &dst,
                                  uint32_t tw, uint32_t th, uint32_t ncomp, const ShiftArr &shift, int32_t mct,
                                  int32_t irrev, hipStream_t s) {
    // interleaved and / or big-endian sources: the loaders for those layouts
    if (fmt & ~0xff) return launch_dcshift_mct_fwd_from(src, fmt, sstride, dst, tw, tw, th, ncomp, shift, mct, irrev, s);
    dim3 grid((tw + 255) / 256, th);
    // Non-temporal output stores: with plain stores the 8 B/sample this pass
    // writes sit dirty in L2 / MALL and are written back while the first DWT
    // level runs, which then reads at ~4 TB/s instead of ~6
    // (scripts/probe/read_pattern.hip "dirty 1").  Measured on the 8K frame:
    // MCT 0.137 -> 0.150 ms, 9/7 DWT 0.255 -> 0.239.
#define GRK_DCS(S) hipLaunchKernelGGL((k_dcshift_mct_fwd<true, S>), grid, dim3(256), 0, s, src, sstride, dst, tw, th, \
                                      ncomp, shift, mct, irrev)
    switch (fmt) {
        case SMP_I32: GRK_DCS(int32_t); break;
        case SMP_U8: GRK_DCS(uint8_t); break;
        case SMP_I8: GRK_DCS(int8_t); break;
        case SMP_U16: GRK_DCS(uint16_t); break;
        case SMP_I16: GRK_DCS(int16_t); break;
        default: return hipErrorInvalidValue;
    }
#undef GRK_DCS
    return hipGetLastError();
}

hipError_t launch_dcshift_mct_custom(const SrcPlanes &src, int32_t fmt, uint32_t sstride, const PlanePtrs &dst,
                                     uint32_t tw, uint32_t th, uint32_t ncomp, const ShiftArr &shift,
                                     const MctMatrix &m, hipStream_t s) {
    if (ncomp > GRK_MAX_COMPS) return hipErrorInvalidValue;
    dim3 grid((tw + 255) / 256, th);
    const int M = src_mode(fmt, ncomp);
    if (M < 0) return hipErrorInvalidValue;
#define GRK_DCM(S, MM) hipLaunchKernelGGL((k_dcshift_mct_custom<S, MM>), grid, dim3(256), 0, s, src, sstride, dst, tw, th, \
                                          ncomp, shift, m)
#define GRK_DCC(S) \
    if (M == 0) GRK_DCM(S, 0); \
    else GRK_DCM(S, 2)
#define GRK_DCC16(S) \
    if (M == 0) GRK_DCM(S, 0); \
    else if (M == 1) GRK_DCM(S, 1); \
    else if (M == 2) GRK_DCM(S, 2); \
    else GRK_DCM(S, 3)
    switch (fmt & 0xff) {
        case SMP_I32: GRK_DCC(int32_t); break;
        case SMP_U8: GRK_DCC(uint8_t); break;
        case SMP_I8: GRK_DCC(int8_t); break;
        case SMP_U16: GRK_DCC16(uint16_t); break;
        case SMP_I16: GRK_DCC16(int16_t); break;
        default: return hipErrorInvalidValue;
    }
#undef GRK_DCC16
#undef GRK_DCC
#undef GRK_DCM
    return hipGetLastError();
}

template <typename S, bool BE>
static void launch_fwd_from(const SrcPlanes &src, bool il, uint32_t sstride, const PlanePtrs &dst, uint32_t dstride,
                            uint32_t tw, uint32_t th, uint32_t ncomp, const ShiftArr &shift, int32_t mct, int32_t irrev,
                            hipStream_t s) {
    mct = mct && ncomp >= 3;
    if (il && (ncomp == 3 || ncomp == 4)) {
        // threads of a row: the lead run + the runs of N pixels
        const uint32_t runs = (uint32_t)(((uint64_t)tw + PIX_RUN - 1) / PIX_RUN + 1);
        const dim3 grid((runs + 255) / 256, th);
        if (ncomp == 3)
            hipLaunchKernelGGL((k_dcshift_mct_fwd_pixels<S, 3, BE>), grid, dim3(256), 0, s, src, sstride, dst, dstride, tw,
                               th, shift, mct, irrev);
        else
            hipLaunchKernelGGL((k_dcshift_mct_fwd_pixels<S, 4, BE>), grid, dim3(256), 0, s, src, sstride, dst, dstride, tw,
                               th, shift, mct, irrev);
        return;
    }
    const dim3 grid((tw + 255) / 256, th);
    if (il)
        hipLaunchKernelGGL((k_dcshift_mct_fwd_from<S, 2 | (BE ? 1 : 0)>), grid, dim3(256), 0, s, src, sstride, dst,
                           dstride, tw, th, ncomp, shift, mct, irrev);
    else
        hipLaunchKernelGGL((k_dcshift_mct_fwd_from<S, BE ? 1 : 0>), grid, dim3(256), 0, s, src, sstride, dst, dstride, tw,
                           th, ncomp, shift, mct, irrev);
}

hipError_t launch_dcshift_mct_fwd_from(const SrcPlanes &src, int32_t fmt, uint32_t sstride, const PlanePtrs &dst,
                                       uint32_t dstride, uint32_t tw, uint32_t th, uint32_t ncomp,
                                       const ShiftArr &shift, int32_t mct, int32_t irrev, hipStream_t s) {
    if (ncomp < 1 || ncomp > (uint32_t)GRK_MAX_COMPS) return hipErrorInvalidValue;
    const int M = src_mode(fmt, ncomp);
    if (M < 0) return hipErrorInvalidValue;
    if (!tw || !th) return hipSuccess;
    const bool il = (M & 2) != 0;
#define GRK_FROM(S, BE) launch_fwd_from<S, BE>(src, il, sstride, dst, dstride, tw, th, ncomp, shift, mct, irrev, s)
    switch (fmt & 0xff) {
        case SMP_I32: GRK_FROM(int32_t, false); break;
        case SMP_U8: GRK_FROM(uint8_t, false); break;
        case SMP_I8: GRK_FROM(int8_t, false); break;
        case SMP_U16: if (M & 1) GRK_FROM(uint16_t, true); else GRK_FROM(uint16_t, false); break;
        case SMP_I16: if (M & 1) GRK_FROM(int16_t, true); else GRK_FROM(int16_t, false); break;
        default: return hipErrorInvalidValue;
    }
#undef GRK_FROM
    return hipGetLastError();
}

hipError_t launch_mct_inv_dcshift(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th,
                                  const PlanePtrs &dst, uint32_t dstride, uint32_t ncomp, const ShiftArr &shift,
                                  const ShiftArr &mn, const ShiftArr &mx, int32_t mct, int32_t irrev, hipStream_t s) {
    dim3 grid((tw + 255) / 256, th);
    hipLaunchKernelGGL(k_mct_inv_dcshift, grid, dim3(256), 0, s, src, sstride, tw, th, dst, dstride, ncomp, shift, mn,
                       mx, mct, irrev);
    return hipGetLastError();
}

// The narrowing store of one tile with the ops of class OP (none, or one
// OutOps) as the kernels' trailing pack.  sYCC / eYCC have three components
// and CMYK four or more (checked by the callers).
template <typename T, int OP = 0, typename... O>
static void launch_inv(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th, const DstPlanes &dst,
                       bool interleaved, uint32_t dstride, uint32_t ncomp, const ShiftArr &shift, const ShiftArr &mn,
                       const ShiftArr &mx, int32_t mct, int32_t irrev, hipStream_t s, const O &...ops) {
    const dim3 grid = run_grid<T>(tw, th);
    mct = mct && ncomp >= 3;
    // nc...: the planar and any-count kernels' ncomp argument
    const auto run = [&](auto kernel, dim3 g, auto... nc) {
        hipLaunchKernelGGL(kernel, g, dim3(256), 0, s, src, sstride, tw, th, dst, dstride, nc..., shift, mn, mx, mct,
                           irrev, ops...);
    };
    if constexpr (op_ycc(OP)) {
        if (!interleaved) run(k_mct_inv_dcshift_planar<T, OP, O...>, grid, ncomp);
        else run(k_mct_inv_dcshift_pixels<T, 3, OP, O...>, grid);
    } else if constexpr (OP == OP_CMYK) {  // one channel fewer than components
        if (!interleaved) run(k_mct_inv_dcshift_planar<T, OP, O...>, grid, ncomp);
        else if (ncomp == 4) run(k_mct_inv_dcshift_pixels<T, 4, OP, O...>, grid);
        else if (ncomp == 5) run(k_mct_inv_dcshift_pixels<T, 5, OP, O...>, grid);
        else run(k_mct_inv_dcshift_pixels_any<T, OP, O...>, pixel_grid(tw, th), ncomp);
    } else {
        if (!interleaved || ncomp == 1) run(k_mct_inv_dcshift_planar<T, OP, O...>, grid, ncomp);
        else if (ncomp == 3) run(k_mct_inv_dcshift_pixels<T, 3, OP, O...>, grid);
        else if (ncomp == 4) run(k_mct_inv_dcshift_pixels<T, 4, OP, O...>, grid);
        else run(k_mct_inv_dcshift_pixels_any<T, OP, O...>, pixel_grid(tw, th), ncomp);
    }
}

hipError_t launch_mct_inv_dcshift_to(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th,
                                     const DstPlanes &dst, int32_t fmt, bool interleaved, uint32_t dstride,
                                     uint32_t ncomp, const ShiftArr &shift, const ShiftArr &mn, const ShiftArr &mx,
                                     int32_t mct, int32_t irrev, hipStream_t s) {
    if (ncomp < 1 || ncomp > (uint32_t)GRK_MAX_COMPS) return hipErrorInvalidValue;
    if (!tw || !th) return hipSuccess;
    if (fmt == SMP_I32 && !interleaved) {  // int32 planes: the kernel every int32 decode has always run
        PlanePtrs d{};
        for (uint32_t k = 0; k < ncomp; ++k) d.p[k] = (int32_t *)dst.p[k];
        return launch_mct_inv_dcshift(src, sstride, tw, th, d, dstride, ncomp, shift, mn, mx, mct, irrev, s);
    }
    return with_sample_type(fmt, [&](auto t) {
        launch_inv<decltype(t)>(src, sstride, tw, th, dst, interleaved, dstride, ncomp, shift, mn, mx, mct, irrev, s);
    });
}

// ---------------------------------------------------------------------------
// The same store for a table of tiles (StoreJob, grk_device.h) in one launch:
// the batch decode's last stage, where one launch per tile would cost more
// than the tiles' samples.  Workgroup wg belongs to the last job j with
// first[j] <= wg (first: the jobs' first workgroup numbers, njobs + 1 entries,
// an empty job's equal to its successor's, so it is never found).  The search
// depends on blockIdx alone: it, the record's fields and the job's OutOps are
// uniform over the workgroup, read with scalar loads before the first store
// and kept in scalar registers.  Thread g of a job -- g counted over its
// workgroups -- owns run (g % rpr) of row (g / rpr), rpr =
// store_job_row_threads: store_planar_run / store_pixels_run's run on the
// destination's 16-byte grid, or (IL with two components) store_pixel_any's
// pixel -- the bodies the per-tile kernels call.  No LDS, no atomics, nothing
// shared between workgroups.
//
// OP and the trailing pack are the per-tile kernels': OP = 0 takes no further
// argument, any other OP the device table of OutOps that StoreJob::ops
// indexes.  OP_SYCC / OP_EYCC jobs have three components, OP_CMYK jobs four.
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t job_of_wg(const uint32_t *__restrict__ first, uint32_t njobs, uint32_t wg) {
    uint32_t lo = 0, hi = njobs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (first[mid] <= wg) lo = mid; else hi = mid;
    }
    return lo;
}

using OpsTable = const OutOps *__restrict__;
__device__ __forceinline__ const OutOps *job_ops(uint32_t) { return nullptr; }
__device__ __forceinline__ const OutOps *job_ops(uint32_t i, OpsTable tab) { return tab + i; }

template <typename T, bool IL, int OP = 0, typename... O>
__global__ void __launch_bounds__(256) k_store_jobs(const StoreJob *__restrict__ jobs,
                                                    const uint32_t *__restrict__ first, uint32_t njobs, O... opstab) {
    static_assert(sizeof...(O) == (OP != 0), "the OutOps table exactly when OP != 0");
    const uint32_t wg = blockIdx.x;
    const uint32_t lo = job_of_wg(first, njobs, wg);
    const StoreJob J = jobs[lo];
    const OutOps *const ops = job_ops(J.ops, opstab...);
    const uint32_t ncomp = op_ycc(OP) ? 3u : (OP == OP_CMYK ? 4u : J.ncomp), tw = J.w, th = J.h;
    const int32_t mct = J.mct && ncomp >= 3, irrev = (int32_t)J.irrev;
    PlanePtrs src{};
    DstPlanes dst{};
    ShiftArr shift{}, minv{}, maxv{};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        src.p[k] = const_cast<int32_t *>(J.src[k]); dst.p[k] = J.dst[k];
        shift.v[k] = J.shift[k]; minv.v[k] = J.mn[k]; maxv.v[k] = J.mx[k];
    }
    const uint32_t rpr = store_job_row_threads(tw, ncomp, (uint32_t)sizeof(T), IL);
    const uint32_t g = (wg - first[lo]) * 256u + threadIdx.x;
    const uint32_t y = g / rpr, t = g - y * rpr;
    if (y >= th) return;
    if constexpr (IL) {
        if constexpr (op_ycc(OP) || OP == OP_CMYK) {
            store_pixels_run<T, OP == OP_CMYK ? 4 : 3, OP>(src, J.sstride, tw, J.dst[0], J.dstride, y, t, shift, minv, maxv,
                                                           mct, irrev, ops);
            return;
        } else {
            if (ncomp == 3) {
                store_pixels_run<T, 3, OP>(src, J.sstride, tw, J.dst[0], J.dstride, y, t, shift, minv, maxv, mct, irrev, ops);
                return;
            }
            if (ncomp == 4) {
                store_pixels_run<T, 4, OP>(src, J.sstride, tw, J.dst[0], J.dstride, y, t, shift, minv, maxv, mct, irrev, ops);
                return;
            }
            if (ncomp == 2) {  // a thread per pixel, a store per sample
                store_pixel_any<T, OP, 4>(src, J.sstride, J.dst[0], J.dstride, 2u, y, t, shift, minv, maxv, 0, irrev, ops);
                return;
            }
        }
    }
    // planar (one interleaved component is a plane)
    store_planar_run<T, OP, 4>(src, J.sstride, tw, dst, J.dstride, ncomp, y, t, shift, minv, maxv, mct, irrev, ops);
}

hipError_t launch_store_jobs(const StoreJob *jobs, const uint32_t *first, uint32_t njobs, uint32_t nwg, int32_t fmt,
                             bool interleaved, hipStream_t s, int op, const OutOps *ops) {
    if (!njobs || !nwg) return hipSuccess;
    if (op < 0 || op > OP_CMYK || (op != 0) != (ops != nullptr)) return hipErrorInvalidValue;
    if (op > OP_PREC && !colour_fmt_of(fmt)) return hipErrorInvalidValue;
    if (op == 0 && float_fmt(fmt)) return hipErrorInvalidValue;  // a float store always has its OutOps
    return with_out_type(fmt, [&](auto t) {
        using T = decltype(t);
        // (the table's type is spelled out: deduced from `ops` it would lose its __restrict__)
        const auto launch = [&](auto c, auto il) {
            constexpr int OP = decltype(c)::value;
            constexpr bool IL = decltype(il)::value != 0;
            if constexpr (OP == 0)
                hipLaunchKernelGGL((k_store_jobs<T, IL>), dim3(nwg), dim3(256), 0, s, jobs, first, njobs);
            else
                hipLaunchKernelGGL((k_store_jobs<T, IL, OP, OpsTable>), dim3(nwg), dim3(256), 0, s, jobs, first, njobs,
                                   ops);
        };
        const auto layouts = [&](auto c) {
            if (interleaved) launch(c, Const<1>{});
            else launch(c, Const<0>{});
        };
        if constexpr (!float_tag<T>) {
            if (op == 0) return layouts(Const<0>{});
        }
        if constexpr (colour_fmt<T>) {
            if (op == OP_SYCC) return layouts(Const<OP_SYCC>{});
            if (op == OP_EYCC) return layouts(Const<OP_EYCC>{});
            if (op == OP_CMYK) return layouts(Const<OP_CMYK>{});
        }
        layouts(Const<OP_PREC>{});
    });
}

// ---------------------------------------------------------------------------
// The DC shift + forward MCT of a table of tiles in one launch (the batch
// encode: a few workgroups per tile, hundreds of tiles) -- the forward mirror
// of k_store_jobs.  Workgroup wg finds its job with job_of_wg; the search
// depends on blockIdx alone, so it and the job record are wave-uniform: scalar
// loads, the record in scalar registers.  Thread g of a job -- g counted over its workgroups -- owns
// position (g % rpr) of row (g / rpr), rpr = load_job_row_threads: a run of
// PIX_RUN pixels of an interleaved 3 / 4-component source
// (k_dcshift_mct_fwd_pixels' runs on the source row's best aligned grid, read
// and stored by the same helpers), else one sample position
// (k_dcshift_mct_fwd's typed loads for planar samples in host byte order,
// k_dcshift_mct_fwd_from's byte-addressed ones otherwise), the arithmetic
// statement for statement.  Rows are packed into the workgroups, so a 64-wide
// tile fills its wavefronts where a (tw / 256, th) grid leaves three quarters
// of each idle.  Stores are non-temporal as there.  No LDS, no atomics,
// nothing shared between workgroups.
// M: bit 0 = big-endian samples, bit 1 = interleaved.
// ---------------------------------------------------------------------------
template <typename S, int NC, bool BE>
__device__ __forceinline__ void load_job_pixels(const LoadJob &J, uint32_t y, uint32_t t, const int32_t (&shift)[4],
                                                int32_t mct, int32_t irrev) {
    constexpr int N = PIX_RUN;
    const uint8_t *const srow = (const uint8_t *)J.src[0] + (size_t)y * J.sstride * sizeof(S);
    uint32_t x0;
    const int n = src_run_of<N>((uintptr_t)srow, NC * sizeof(S), t, J.w, x0);
    if (n <= 0) return;
    int32_t px[N * NC];
    load_samples<S, N * NC, BE>(srow + (size_t)x0 * NC * sizeof(S), px, n * NC);
    int32_t v[NC][N];
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int k = 0; k < NC; ++k) v[k][i] = px[i * NC + k];
    if (mct) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            int32_t r = v[0][i] - shift[0], g = v[1][i] - shift[1], b = v[2][i] - shift[2];
            int32_t o0, o1, o2;
            if (!irrev) {
                o0 = (r + (g * 2) + b) >> 2;
                o1 = b - g;
                o2 = r - g;
            } else {
                o0 = ict_term(r, 2449) + ict_term(g, 4809) + ict_term(b, 934);
                o1 = -ict_term(r, 1382) - ict_term(g, 2714) + ict_term(b, 4096);
                o2 = ict_term(r, 4096) - ict_term(g, 3430) - ict_term(b, 666);
            }
            v[0][i] = o0; v[1][i] = o1; v[2][i] = o2;
        }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        if (mct && k < 3) continue;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            int32_t s = v[k][i] - shift[k];
            v[k][i] = irrev ? (int32_t)((uint32_t)s << 11) : s;
        }
    }
    const size_t di = (size_t)y * J.dstride + x0;
#pragma unroll
    for (int k = 0; k < NC; ++k) store_run<N>(J.dst[k] + di, v[k], n);
}

template <typename S, int M>
__global__ void __launch_bounds__(256) k_load_jobs(const LoadJob *__restrict__ jobs,
                                                   const uint32_t *__restrict__ first, uint32_t njobs) {
    constexpr bool BE = (M & 1) != 0, IL = (M & 2) != 0;
    const uint32_t wg = blockIdx.x;
    const uint32_t lo = job_of_wg(first, njobs, wg);
    const LoadJob J = jobs[lo];
    const uint32_t ncomp = J.ncomp, tw = J.w, th = J.h;
    const int32_t mct = J.mct && ncomp >= 3, irrev = J.irrev;
    int32_t shift[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) shift[k] = J.shift[k];
    const uint32_t rpr = load_job_row_threads(tw, ncomp, IL);
    const uint32_t g = (wg - first[lo]) * 256u + threadIdx.x;
    const uint32_t y = g / rpr, x = g - y * rpr;
    if (y >= th) return;
    if constexpr (IL) {
        if (ncomp == 3) { load_job_pixels<S, 3, BE>(J, y, x, shift, mct, irrev); return; }
        if (ncomp == 4) { load_job_pixels<S, 4, BE>(J, y, x, shift, mct, irrev); return; }
    }
    // one sample position, one load per component
    const size_t srow = (size_t)y * J.sstride, di = (size_t)y * J.dstride + x;
    int32_t v[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((uint32_t)k >= ncomp) continue;
        if constexpr (M == 0) {
            v[k] = (int32_t)((const S *)J.src[k])[srow + x];
        } else {
            const uint8_t *p = IL ? (const uint8_t *)J.src[0] + (srow + (size_t)x * ncomp + k) * sizeof(S)
                                  : (const uint8_t *)J.src[k] + (srow + x) * sizeof(S);
            v[k] = ld_sample<S, BE>(p);
        }
    }
    if (mct) {
        int32_t r = v[0] - shift[0], gg = v[1] - shift[1], b = v[2] - shift[2];
        int32_t o0, o1, o2;
        if (!irrev) {
            o0 = (r + (gg * 2) + b) >> 2;
            o1 = b - gg;
            o2 = r - gg;
        } else {
            o0 = ict_term(r, 2449) + ict_term(gg, 4809) + ict_term(b, 934);
            o1 = -ict_term(r, 1382) - ict_term(gg, 2714) + ict_term(b, 4096);
            o2 = ict_term(r, 4096) - ict_term(gg, 3430) - ict_term(b, 666);
        }
        put<true>(&J.dst[0][di], o0); put<true>(&J.dst[1][di], o1); put<true>(&J.dst[2][di], o2);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if ((uint32_t)k >= ncomp || (mct && k < 3)) continue;
        const int32_t s = v[k] - shift[k];
        put<true>(&J.dst[k][di], irrev ? (int32_t)((uint32_t)s << 11) : s);
    }
}

hipError_t launch_load_jobs(const LoadJob *jobs, const uint32_t *first, uint32_t njobs, uint32_t nwg, int32_t fmt,
                            int mode, hipStream_t s) {
    if (!njobs || !nwg) return hipSuccess;
    if (mode < 0 || mode > 3) return hipErrorInvalidValue;
    if ((mode & 1) && fmt != SMP_U16 && fmt != SMP_I16) return hipErrorInvalidValue;  // big-endian: 16-bit samples only
    return with_sample_type(fmt, [&](auto t) {
        using S = decltype(t);
        const auto run = [&](auto m) {
            hipLaunchKernelGGL((k_load_jobs<S, decltype(m)::value>), dim3(nwg), dim3(256), 0, s, jobs, first, njobs);
        };
        if constexpr (sizeof(S) == 2) {
            if (mode == 1) return run(Const<1>{});
            if (mode == 3) return run(Const<3>{});
        }
        if (mode & 2) run(Const<2>{});
        else run(Const<0>{});
    });
}

// The upsampling store of one rectangle with the ops of class OP (none, or one
// OutOps) as the kernels' trailing pack.  fast: conv_job_fast's shape, which
// runs k_upsample_420 (OP_SYCC only there); everything else runs
// k_upsample_any, which reads its colour step from the ops at run time.
template <typename T, int OP = 0, typename... O>
static void launch_up(const UpPlan &src, uint32_t ncomp, uint32_t X0, uint32_t Y0, uint32_t w, uint32_t h,
                      const DstPlanes &dst, bool interleaved, uint32_t dstride, bool fast, hipStream_t s,
                      const O &...ops) {
    if constexpr (colour_fmt<T>) {
        if (fast) {
            if (interleaved)
                hipLaunchKernelGGL((k_upsample_420<T, true, OP, O...>), run_grid<T>(w, h), dim3(256), 0, s, src, X0, Y0,
                                   w, h, dst, dstride, ops...);
            else
                hipLaunchKernelGGL((k_upsample_420<T, false, OP, O...>), run_grid<T>(w, h), dim3(256), 0, s, src, X0, Y0,
                                   w, h, dst, dstride, ops...);
            return;
        }
    }
    hipLaunchKernelGGL((k_upsample_any<T, OP ? OP_PREC : 0, O...>), pixel_grid(w, h), dim3(256), 0, s, src, ncomp, X0,
                       Y0, w, h, dst, interleaved ? 1 : 0, dstride, ops...);
}

hipError_t launch_upsample_to(const UpPlan &src, uint32_t ncomp, uint32_t X0, uint32_t Y0, uint32_t w, uint32_t h,
                              const DstPlanes &dst, int32_t fmt, bool interleaved, uint32_t dstride, hipStream_t s) {
    if (ncomp < 1 || ncomp > (uint32_t)GRK_MAX_COMPS) return hipErrorInvalidValue;
    for (uint32_t k = 0; k < ncomp; ++k)
        if (!src.c[k].dx || !src.c[k].dy) return hipErrorInvalidValue;
    if (!w || !h) return hipSuccess;
    const bool fast = conv_job_fast(src.c, ncomp, fmt, COL_NONE);
    return with_sample_type(fmt, [&](auto t) {
        launch_up<decltype(t)>(src, ncomp, X0, Y0, w, h, dst, interleaved, dstride, fast, s);
    });
}

// sYCC / eYCC / CMYK output is unsigned: its formats are U8 / U16 / I32
static bool sycc_launchable(const OutOps &ops, uint32_t ncomp, int32_t fmt) {
    if (ops.col != COL_NONE && (ops.sycc || (ops.col != COL_EYCC && ops.col != COL_CMYK))) return false;
    if (!ops.sycc && ops.col == COL_NONE) return true;
    return (ops.col == COL_CMYK ? ncomp >= 4 : ncomp == 3) && colour_fmt_of(fmt);
}

// the same launches with the OutOps in their stores
hipError_t launch_mct_inv_dcshift_ops(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th,
                                      const DstPlanes &dst, int32_t fmt, bool interleaved, uint32_t dstride,
                                      uint32_t ncomp, const ShiftArr &shift, const ShiftArr &mn, const ShiftArr &mx,
                                      int32_t mct, int32_t irrev, const OutOps &ops, hipStream_t s) {
    if (ncomp < 1 || ncomp > (uint32_t)GRK_MAX_COMPS || !sycc_launchable(ops, ncomp, fmt))
        return hipErrorInvalidValue;
    if (!tw || !th) return hipSuccess;
    return with_out_type(fmt, [&](auto t) {
        using T = decltype(t);
        with_op<T>(ops, [&](auto op) {
            launch_inv<T, decltype(op)::value, OutOps>(src, sstride, tw, th, dst, interleaved, dstride, ncomp, shift,
                                                       mn, mx, mct, irrev, s, ops);
        });
    });
}

hipError_t launch_upsample_ops(const UpPlan &src, uint32_t ncomp, uint32_t X0, uint32_t Y0, uint32_t w, uint32_t h,
                               const DstPlanes &dst, int32_t fmt, bool interleaved, uint32_t dstride,
                               const OutOps &ops, hipStream_t s) {
    if (ncomp < 1 || ncomp > (uint32_t)GRK_MAX_COMPS || !sycc_launchable(ops, ncomp, fmt))
        return hipErrorInvalidValue;
    for (uint32_t k = 0; k < ncomp; ++k)
        if (!src.c[k].dx || !src.c[k].dy) return hipErrorInvalidValue;
    if (!w || !h) return hipSuccess;
    // (eYCC / CMYK need one grid, which the fast shape is not: k_upsample_any's)
    const bool fast = conv_job_fast(src.c, ncomp, fmt, ops.col);
    return with_out_type(fmt, [&](auto t) {
        using T = decltype(t);
        if constexpr (colour_fmt<T>) {
            if (fast && ops.sycc)
                return launch_up<T, OP_SYCC, OutOps>(src, ncomp, X0, Y0, w, h, dst, interleaved, dstride, fast, s, ops);
        }
        launch_up<T, OP_PREC, OutOps>(src, ncomp, X0, Y0, w, h, dst, interleaved, dstride, fast, s, ops);
    });
}

// the custom-MCT stores: the grids of launch_inv, the ops (none, or one
// OutOps) as the kernels' trailing pack
template <typename T, int OP, typename... O>
static void launch_custom(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th, const DstPlanes &dst,
                          bool interleaved, uint32_t dstride, uint32_t ncomp, const MctInv &m, const ShiftArr &off,
                          const ShiftArr &mn, const ShiftArr &mx, hipStream_t s, const O &...ops) {
    const dim3 grid = run_grid<T>(tw, th);
#define GRK_CUSTOM(KERNEL, NC, GRID) \
    hipLaunchKernelGGL((KERNEL<T, OP, NC>), GRID, dim3(256), 0, s, src, sstride, tw, th, dst, dstride, ncomp, m, off, \
                       mn, mx, ops...)
    if constexpr (op_ycc(OP)) {  // three components (checked by the caller)
        if (!interleaved) GRK_CUSTOM(k_mct_inv_custom_planar, 3, grid);
        else GRK_CUSTOM(k_mct_inv_custom_pixels, 3, grid);
    } else if constexpr (OP == OP_CMYK) {  // four or more components: the any-count forms
        if (!interleaved) GRK_CUSTOM(k_mct_inv_custom_planar, 0, grid);
        else GRK_CUSTOM(k_mct_inv_custom_pixels, 0, pixel_grid(tw, th));
    } else if (!interleaved || ncomp == 1) {
        if (ncomp == 3) GRK_CUSTOM(k_mct_inv_custom_planar, 3, grid);
        else if (ncomp == 4) GRK_CUSTOM(k_mct_inv_custom_planar, 4, grid);
        else GRK_CUSTOM(k_mct_inv_custom_planar, 0, grid);
    } else if (ncomp == 3) {
        GRK_CUSTOM(k_mct_inv_custom_pixels, 3, grid);
    } else if (ncomp == 4) {
        GRK_CUSTOM(k_mct_inv_custom_pixels, 4, grid);
    } else {
        GRK_CUSTOM(k_mct_inv_custom_pixels, 0, pixel_grid(tw, th));
    }
#undef GRK_CUSTOM
}

hipError_t launch_mct_inv_custom(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th,
                                 const DstPlanes &dst, int32_t fmt, bool interleaved, uint32_t dstride,
                                 uint32_t ncomp, const MctInv &m, const ShiftArr &off, const ShiftArr &mn,
                                 const ShiftArr &mx, const OutOps *ops, hipStream_t s) {
    if (ncomp < 1 || ncomp > (uint32_t)GRK_MAX_COMPS || (ops && !sycc_launchable(*ops, ncomp, fmt)))
        return hipErrorInvalidValue;
    if (!tw || !th) return hipSuccess;
    return with_sample_type(fmt, [&](auto t) {
        using T = decltype(t);
        if (!ops) return launch_custom<T, 0>(src, sstride, tw, th, dst, interleaved, dstride, ncomp, m, off, mn, mx, s);
        with_op<T>(*ops, [&](auto op) {
            launch_custom<T, decltype(op)::value>(src, sstride, tw, th, dst, interleaved, dstride, ncomp, m, off, mn,
                                                  mx, s, *ops);
        });
    });
}

// the palette stores: launch_inv's run grid over PAL_ROWS rows per
// workgroup, the table's bytes as dynamic LDS
template <typename T, int OP, typename... O>
static void launch_pal(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th, const DstPlanes &dst,
                       bool interleaved, uint32_t dstride, uint32_t ncomp, const ShiftArr &shift, const ShiftArr &mn,
                       const ShiftArr &mx, int32_t mct, int32_t irrev, const PalMap &map, const uint16_t *table,
                       hipStream_t s, const O &...ops) {
    const uint32_t rows = (th + PAL_ROWS - 1) / PAL_ROWS;
    const dim3 grid = run_grid<T>(tw, rows);
    const size_t lds = ((size_t)map.ne * map.npc * 2 + 3) & ~(size_t)3;
#define GRK_PAL(KERNEL, GRID) \
    hipLaunchKernelGGL(KERNEL, GRID, dim3(256), lds, s, src, sstride, tw, th, dst, dstride, ncomp, shift, mn, mx, mct, \
                       irrev, map, table, ops...)
    if (!interleaved || map.nch == 1) GRK_PAL((k_palette_planar<T, OP>), grid);
    else if (map.nch == 3) GRK_PAL((k_palette_pixels<T, 3, OP>), grid);
    else if (map.nch == 4) GRK_PAL((k_palette_pixels<T, 4, OP>), grid);
    else GRK_PAL((k_palette_pixels<T, 0, OP>), pixel_grid(tw, rows));
#undef GRK_PAL
}

hipError_t launch_palette(const PlanePtrs &src, uint32_t sstride, uint32_t tw, uint32_t th, const DstPlanes &dst,
                          int32_t fmt, bool interleaved, uint32_t dstride, uint32_t ncomp, const ShiftArr &shift,
                          const ShiftArr &mn, const ShiftArr &mx, int32_t mct, int32_t irrev, const PalMap &map,
                          const uint16_t *table, const OutOps *ops, hipStream_t s) {
    if (ncomp < 1 || ncomp > (uint32_t)GRK_MAX_COMPS || map.nch < 1 || map.nch > (uint32_t)GRK_MAX_COMPS ||
        map.ne > 1024 || map.npc > (uint32_t)GRK_MAX_COMPS || (ops && (ops->sycc || ops->col)))
        return hipErrorInvalidValue;
    for (uint32_t c = 0; c < map.nch; ++c) {  // every index the kernel forms stays inside the table and the planes
        if (map.comp[c] >= ncomp || !((map.used >> map.comp[c]) & 1)) return hipErrorInvalidValue;
        if (map.pcol[c] >= 0 && (!table || !map.ne || (uint32_t)map.pcol[c] >= map.npc)) return hipErrorInvalidValue;
    }
    if (!tw || !th) return hipSuccess;
    return with_sample_type(fmt, [&](auto t) {
        using T = decltype(t);
        if (!ops) launch_pal<T, 0>(src, sstride, tw, th, dst, interleaved, dstride, ncomp, shift, mn, mx, mct, irrev,
                                   map, table, s);
        else launch_pal<T, OP_PREC>(src, sstride, tw, th, dst, interleaved, dstride, ncomp, shift, mn, mx, mct, irrev,
                                    map, table, s, *ops);
    });
}

// ---------------------------------------------------------------------------
// The palette store for a table of tiles (PalJob, grk_device.h) in one launch:
// the batch decode of JP2 files.  Workgroup wg finds its job with job_of_wg;
// the search depends on blockIdx alone, so it, the record's fields and the
// job's OutOps are uniform over the workgroup: scalar loads before the first
// store, the StoreJob part kept in scalar registers as in k_store_jobs, the
// map indexed where it lies.  Within its job a workgroup owns one band of
// PAL_ROWS rows by one chunk of 256 row threads (pal_job_row_threads: the runs
// of the destination's 16-byte grid, or SHAPE 2's pixels), so the LDS fill is
// amortised exactly as in the per-tile kernels: ne * npc entries from table +
// table_off, once, and only when the job looks up (ne != 0; a direct or
// force-RGB map has no table).  The rows are palette_planar_row /
// palette_pixels_row / palette_pixel_any, the per-tile kernels' bodies.
// map.zero: null sources, entry 0 of each looked-up channel (the tiles a cut
// stream never reached, the margin of a reduced decode).
//
// SHAPE (pal_job_shape): 0 planar, 3 / 4 interleaved runs, 2 interleaved with
// a thread per pixel.  OP = 0 or OP_PREC with the OutOps table, as
// k_store_jobs.  Dynamic LDS is per launch: the host groups the jobs by the
// size class of their table (pal_lds_class: none, <= 4 KB, <= 32 KB).  No
// atomics, nothing shared between workgroups.
// ---------------------------------------------------------------------------
template <typename T, int SHAPE, int OP = 0, typename... O>
__global__ void __launch_bounds__(256) k_palette_jobs(const PalJob *__restrict__ jobs,
                                                      const uint32_t *__restrict__ first, uint32_t njobs,
                                                      const uint16_t *__restrict__ table, O... opstab) {
    static_assert(sizeof...(O) == (OP != 0), "the OutOps table exactly when OP != 0");
    static_assert(OP == 0 || OP == OP_PREC, "no colour conversion behind a palette");
    extern __shared__ uint16_t pal_lut[];
    const uint32_t wg = blockIdx.x;
    const uint32_t lo = job_of_wg(first, njobs, wg);
    const StoreJob J = jobs[lo].s;
    const PalMap &map = jobs[lo].map;
    const OutOps *const ops = job_ops(J.ops, opstab...);
    if (map.ne) palette_load(pal_lut, table + jobs[lo].table_off, map.ne * map.npc);  // (uniform: every thread or none)
    const uint32_t ncomp = J.ncomp, tw = J.w, th = J.h;
    const int32_t mct = J.mct && ncomp >= 3, irrev = (int32_t)J.irrev;
    PlanePtrs src{};
    DstPlanes dst{};
    ShiftArr shift{}, minv{}, maxv{};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        src.p[k] = const_cast<int32_t *>(J.src[k]); dst.p[k] = J.dst[k];
        shift.v[k] = J.shift[k]; minv.v[k] = J.mn[k]; maxv.v[k] = J.mx[k];
    }
    const uint32_t chunks = (pal_job_row_threads(tw, (uint32_t)sizeof(T), SHAPE) + 255u) / 256u;
    const uint32_t b = wg - first[lo], band = b / chunks;
    const uint32_t t = (b - band * chunks) * 256u + threadIdx.x;
    const uint32_t yb = band * PAL_ROWS, ye = yb + PAL_ROWS < th ? yb + PAL_ROWS : th;
    for (uint32_t y = yb; y < ye; ++y) {
        if constexpr (SHAPE == 3 || SHAPE == 4)
            palette_pixels_row<T, SHAPE, OP, 4>(src, J.sstride, tw, J.dst[0], J.dstride, ncomp, y, t, shift, minv, maxv,
                                                mct, irrev, map, pal_lut, ops);
        else if constexpr (SHAPE == 2)
            palette_pixel_any<T, OP, 4>(src, J.sstride, tw, J.dst[0], J.dstride, ncomp, y, t, shift, minv, maxv, mct, irrev,
                                        map, pal_lut, ops);
        else
            palette_planar_row<T, OP, 4>(src, J.sstride, tw, dst, J.dstride, ncomp, y, t, shift, minv, maxv, mct, irrev,
                                         map, pal_lut, ops);
    }
}

static_assert(PAL_JOB_ROWS == (uint32_t)PAL_ROWS, "pal_job_wgs counts the kernels' bands");
hipError_t launch_palette_jobs(const PalJob *jobs, const uint32_t *first, uint32_t njobs, uint32_t nwg, int32_t fmt,
                               int shape, int op, const OutOps *ops, const uint16_t *table, uint32_t lds_bytes,
                               hipStream_t s) {
    if (!njobs || !nwg) return hipSuccess;
    if ((op != 0 && op != OP_PREC) || (op != 0) != (ops != nullptr) || shape < 0 || shape > 4 || shape == 1 ||
        lds_bytes > 32768 || (lds_bytes && (!table || ((uintptr_t)table & 3))))
        return hipErrorInvalidValue;
    return with_sample_type(fmt, [&](auto t) {
        using T = decltype(t);
        const auto launch = [&](auto sh) {
            constexpr int SHAPE = decltype(sh)::value;
            if (op == 0)
                hipLaunchKernelGGL((k_palette_jobs<T, SHAPE>), dim3(nwg), dim3(256), lds_bytes, s, jobs, first, njobs,
                                   table);
            else
                hipLaunchKernelGGL((k_palette_jobs<T, SHAPE, OP_PREC, OpsTable>), dim3(nwg), dim3(256), lds_bytes, s, jobs,
                                   first, njobs, table, ops);
        };
        if (shape == 0) launch(Const<0>{});
        else if (shape == 2) launch(Const<2>{});
        else if (shape == 3) launch(Const<3>{});
        else launch(Const<4>{});
    });
}

// ---------------------------------------------------------------------------
// launch_upsample_ops for a table of jobs (ConvJob; the batch decode with
// output ops), in its two thread shapes: job_of_wg in front of
// upsample_420_run / upsample_any_pixel.  The job stays in memory: its
// components and destinations are indexed at run time.  No LDS, no atomics,
// nothing shared between workgroups.
// ---------------------------------------------------------------------------
template <typename T, bool IL, int OP>
__global__ void __launch_bounds__(256) k_conv_jobs_420(const ConvJob *__restrict__ jobs,
                                                       const uint32_t *__restrict__ first, uint32_t njobs,
                                                       const OutOps *__restrict__ opstab) {
    const uint32_t wg = blockIdx.x;
    const uint32_t lo = job_of_wg(first, njobs, wg);
    const ConvJob &J = jobs[lo];
    const uint32_t w = J.x1 - J.X0, h = J.y1 - J.Y0;
    const uint32_t rpr = conv_job_row_threads(w, (uint32_t)sizeof(T), true);
    const uint32_t g = (wg - first[lo]) * 256u + threadIdx.x;
    const uint32_t y = g / rpr, t = g - y * rpr;
    if (y >= h) return;
    upsample_420_run<T, IL, OP>(J.c, J.X0, J.Y0, w, t, y, J.dst, J.dstride, opstab + J.ops);
}
template <typename T>
__global__ void __launch_bounds__(256) k_conv_jobs_any(const ConvJob *__restrict__ jobs,
                                                       const uint32_t *__restrict__ first, uint32_t njobs,
                                                       const OutOps *__restrict__ opstab, int32_t il) {
    const uint32_t wg = blockIdx.x;
    const uint32_t lo = job_of_wg(first, njobs, wg);
    const ConvJob &J = jobs[lo];
    const uint32_t w = J.x1 - J.X0, h = J.y1 - J.Y0;
    const uint32_t g = (wg - first[lo]) * 256u + threadIdx.x;
    const uint32_t y = g / w, x = g - y * w;
    if (y >= h) return;
    upsample_any_pixel<T, OP_PREC>(J.c, J.ncomp, J.X0, J.Y0, x, y, J.dst, il, J.dstride, opstab + J.ops);
}

hipError_t launch_conv_jobs(const ConvJob *jobs, const uint32_t *first, uint32_t njobs, uint32_t nwg,
                            const OutOps *ops, int32_t fmt, bool interleaved, bool fast, bool sycc, hipStream_t s) {
    if (!njobs || !nwg) return hipSuccess;
    if (fast && !colour_fmt_of(fmt)) return hipErrorInvalidValue;
    return with_out_type(fmt, [&](auto t) {
        using T = decltype(t);
        if constexpr (colour_fmt<T>) {
            if (fast) {
                const auto run = [&](auto il, auto op) {
                    hipLaunchKernelGGL((k_conv_jobs_420<T, decltype(il)::value != 0, decltype(op)::value>), dim3(nwg),
                                       dim3(256), 0, s, jobs, first, njobs, ops);
                };
                if (interleaved && sycc) run(Const<1>{}, Const<OP_SYCC>{});
                else if (interleaved) run(Const<1>{}, Const<OP_PREC>{});
                else if (sycc) run(Const<0>{}, Const<OP_SYCC>{});
                else run(Const<0>{}, Const<OP_PREC>{});
                return;
            }
        }
        hipLaunchKernelGGL(k_conv_jobs_any<T>, dim3(nwg), dim3(256), 0, s, jobs, first, njobs, ops,
                           interleaved ? 1 : 0);
    });
}

// MQ encoder: 64 blocks (lanes) per wavefront.  The coder is a serial chain
// per block, so throughput = resident blocks / block time: 64 lanes per
// wavefront keep 4x more blocks resident per wave slot than 16.
constexpr int MQ_LANES = 64;
constexpr int MQ_WAVES = 4;  // wavefronts per MQ-coder workgroup
// T1 decoder: 64 blocks (lanes) per wavefront, same reasoning (8K frame batch,
// 12 frames in flight: 2.0-2.2 vs 1.25 Gpix/s with 16; a lone frame decodes
// ~10% faster with 16).
constexpr int DEC_LANES = 64;

// Blocks per wavefront of the lane coders: 64 keeps the most blocks resident
// per wave slot, which is what the throughput of many frames in flight
// needs; a launch of few blocks (a small image) is bound by its longest
// block's chain instead, and the 64 blocks of a wavefront execute the union of
// their paths -- there one block per wavefront (n <= 1024: at most one
// wavefront per SIMD), then 2, 4, ... up to 64 from 4096 blocks on.
uint32_t lone_bpw(uint32_t n) {
    uint32_t b = 1;
    while (b < 64 && (uint64_t)n >= 1536ull * (2 * b)) b <<= 1;
    return b;
}

static uint32_t t1_blocks_per_wave(uint32_t n) {
    uint32_t b = 1;
    while (b < 64 && (uint64_t)n > 1024ull * b) b <<= 1;
    return n >= 4096 ? 64 : b;
}

uint32_t t1_order_words(uint32_t n) { return 2 * n + MQ_ORDER_BUCKETS; }

hipError_t launch_t1_encode(const EncBlock *blocks, uint32_t n, const int32_t *coef, void *scratch_v,
                            uint8_t *sym, const uint64_t *sym_off, uint32_t maxdepth, uint8_t *out, EncResult *res,
                            hipStream_t s, uint32_t cblksty, uint32_t bpw_req, uint32_t *order) {
    if (!n) return hipSuccess;
    uint8_t *scratch = (uint8_t *)scratch_v;
    if (maxdepth > 32) maxdepth = 32;
    if (maxdepth < 1) maxdepth = 1;
    const uint32_t groups8 = (t1_scratch_records(n) / 64 + 7) & ~7u;  // k_t1_prep's XCD deal: whole rounds of 8 groups
    hipLaunchKernelGGL(k_t1_prep, dim3(groups8 * 64), dim3(64), 0, s, blocks, n, maxdepth, coef, scratch, res);
    const uint64_t threads = (uint64_t)t1_scratch_records(n) * maxdepth;
    hipLaunchKernelGGL(k_t1_model<true>, dim3((uint32_t)(threads / 64)), dim3(64), 0, s, blocks, n, maxdepth, scratch,
                       sym, sym_off, res, cblksty);
    const uint32_t bpw = dwt_options().t1_enc_bpw ? (uint32_t)dwt_options().t1_enc_bpw
                         : bpw_req                ? bpw_req
                                                  : t1_blocks_per_wave(n);
    const uint32_t *perm = nullptr;
    const uint32_t *cnt = enc_scratch(scratch, n, maxdepth).cnt;
    if (order && dwt_options().t1_enc_sort && n > 64) {  // order: t1_order_words(n) words
        uint32_t *key = order, *permw = order + n, *hist = order + 2 * n;
        const hipError_t e = hipMemsetAsync(hist, 0, MQ_ORDER_BUCKETS * 4, s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_mq_order_hist, dim3((n + 255) / 256), dim3(256), 0, s, cnt, res, n, key, hist);
        hipLaunchKernelGGL(k_mq_order_scan, dim3(1), dim3(MQ_ORDER_BUCKETS), 0, s, hist);
        hipLaunchKernelGGL(k_mq_order_scatter, dim3((n + 255) / 256), dim3(256), 0, s, key, n, hist, permw);
        perm = permw;
    }
    // Concurrent calls: MQ_WAVES wavefronts per workgroup, 19 context words
    // per lane -- LDS no longer holds the coder at 7 wavefronts per SIMD (5.7
    // KB per single-wavefront workgroup); 8 per SIMD by registers and LDS: 8K
    // batch 3519 / 3476 -> 3664 / 3577 Mpixels/s alternating (profiles/r05/
    // t1_mq_wg_ab.txt).  A call alone on the GPU or a small launch keeps one
    // wavefront per workgroup: its lanes' chains run on separate CUs instead of
    // four wavefronts sharing one CU's LDS -- the 512^2 image's coder took
    // 6.8 ms in 4-wavefront workgroups against 4.1 (profiles/r05/
    // rocprof_512_r4_r5.txt)
    const uint32_t nwv = (n + bpw - 1) / bpw, nwg = (nwv + MQ_WAVES - 1) / MQ_WAVES;
    const bool wide = !bpw_req && n > 4096;
    if (wide && (cblksty & CBLKSTY_LAZY))
        hipLaunchKernelGGL((k_t1_mq<MQ_LANES, 1, true, MQ_WAVES, 19>), dim3(nwg), dim3(MQ_LANES * MQ_WAVES), 0, s,
                           blocks, n, cnt, sym, sym_off, out, res, perm, cblksty, bpw);
    else if (wide)
        hipLaunchKernelGGL((k_t1_mq<MQ_LANES, 1, false, MQ_WAVES, 19>), dim3(nwg), dim3(MQ_LANES * MQ_WAVES), 0, s,
                           blocks, n, cnt, sym, sym_off, out, res, perm, cblksty, bpw);
    else if (cblksty & CBLKSTY_LAZY)
        hipLaunchKernelGGL((k_t1_mq<MQ_LANES, 1, true>), dim3(nwv), dim3(MQ_LANES), 0, s, blocks, n, cnt, sym, sym_off,
                           out, res, perm, cblksty, bpw);
    else
        hipLaunchKernelGGL((k_t1_mq<MQ_LANES, 1, false>), dim3(nwv), dim3(MQ_LANES), 0, s, blocks, n, cnt, sym, sym_off,
                           out, res, perm, cblksty, bpw);
    return hipGetLastError();
}

// t1_generate_luts.cpp:290-318: floor((u^2 - v^2) * 2^6 + 0.5) / 2^6 * 8192
// with t = i / 2^6, clamped at 0 (host double arithmetic, as generated)
static NmseLut make_nmse_lut() {
    NmseLut L;
    for (int i = 0; i < 128; ++i) {
        const double t = i / 64.0;
        double u = t, v = t - 1.5;
        L.sig[i] = (int16_t)std::max(0, (int)(floor((u * u - v * v) * 64.0 + 0.5) / 64.0 * 8192.0));
        L.sig0[i] = (int16_t)std::max(0, (int)(floor((u * u) * 64.0 + 0.5) / 64.0 * 8192.0));
        u = t - 1.0;
        v = (i & 64) ? t - 1.5 : t - 0.5;
        L.ref[i] = (int16_t)std::max(0, (int)(floor((u * u - v * v) * 64.0 + 0.5) / 64.0 * 8192.0));
        L.ref0[i] = (int16_t)std::max(0, (int)(floor((u * u) * 64.0 + 0.5) / 64.0 * 8192.0));
    }
    return L;
}
const NmseLut &nmse_lut() {
    static const NmseLut L = make_nmse_lut();
    return L;
}

hipError_t launch_t1_dist(const EncBlock *blocks, uint32_t n, uint32_t maxdepth, const int32_t *coef,
                          const void *scratch, EncResult *res, hipStream_t s) {
    if (!n) return hipSuccess;
    if (maxdepth > 32) maxdepth = 32;
    if (maxdepth < 1) maxdepth = 1;
    hipLaunchKernelGGL(k_t1_dist, dim3(n), dim3(64), 0, s, blocks, n, maxdepth, coef, (const uint8_t *)scratch, res,
                       nmse_lut());
    return hipGetLastError();
}

// One thread per block (grk_device.h DevPass / PassSum).  The arithmetic is
// the host's, operation for operation in IEEE double (no contraction: the
// library builds with -ffp-contract=off), so the records are bit-identical.
__global__ __launch_bounds__(256) void k_pass_records(const EncBlock *__restrict__ blocks,
                                                      const EncResult *__restrict__ res, const double *__restrict__ wfac,
                                                      const uint64_t *__restrict__ pass0, uint32_t n, uint32_t sty,
                                                      DevPass *__restrict__ out, PassSum *__restrict__ sum) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const EncResult &r = res[i];
    const EncBlock &b = blocks[i];
    PassSum ps{};
    ps.numbps = r.numbps;
    ps.numpasses = r.numpasses;
    ps.len = r.len;
    ps.nsym = r.nsym;
    const uint64_t p0 = pass0[i], cap = pass0[i + 1] - p0;
    uint32_t np = r.numpasses;
    if (r.pad) ps.bad |= 1u;
    if (np > cap || np > GRK_MAX_PASSES) { ps.bad |= 2u; np = 0; }
    if (np && r.rate[np - 1] > t1_enc_slab_bytes(b.w, b.h, sty, r.numbps)) ps.bad |= 4u;
    if (ps.bad) np = 0;
    const double f = wfac[i];
    double cum = 0.0, mn = DBL_MAX, mx = -1, m0 = -HUGE_VAL;
    uint32_t prev = 0, z0 = 0;
    double prevdd = 0.0;
    DevPass *o = out + p0;
    for (uint32_t k = 0; k < np; ++k) {
        DevPass d;
        d.rate = r.rate[k];
        d.len = d.rate - prev;
        const int32_t bp = k == 0 ? (int32_t)r.numbps - 1 : (int32_t)r.numbps - 2 - (int32_t)((k - 1) / 3);
        const int pt = k == 0 ? 2 : (int)((k - 1) % 3);
        d.term = t1_pass_term(sty, bp, pt, r.numbps) ? 1 : 0;
        d.slope = 0;
        // t1_wmsedec_at (t2.h): factor * 2^bpno, squared with nmsedec / 8192
        double w = f * (1 << bp);
        w *= w * r.nmsedec[k] / 8192.0;
        cum += w;
        d.dd = cum;
        o[k] = d;
        // block_slopes (t2.cpp)
        if (d.rate) { const double q = d.dd / d.rate; m0 = m0 < q ? q : m0; }
        else if (d.dd != 0) z0 = 1;
        const int32_t dr = k == 0 ? (int32_t)d.rate : (int32_t)(d.rate - prev);
        const double ddd = k == 0 ? d.dd : d.dd - prevdd;
        if (dr != 0) {
            const double q = ddd / dr;
            if (q < mn) mn = q;
            if (q > mx) mx = q;
        }
        prev = d.rate;
        prevdd = d.dd;
    }
    ps.z0 = z0;
    ps.smin = mn;
    ps.smax = mx;
    ps.s0max = m0;
    ps.disto = cum;
    sum[i] = ps;
}

hipError_t launch_pass_records(const EncBlock *blocks, const EncResult *res, const double *wfac, const uint64_t *pass0,
                               uint32_t n, uint32_t cblksty, DevPass *out, PassSum *sum, hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_pass_records, dim3((n + 255) / 256), dim3(256), 0, s, blocks, res, wfac, pass0, n, cblksty,
                       out, sum);
    return hipGetLastError();
}

hipError_t launch_t1_decode(const DecBlock *blocks, uint32_t n, const uint8_t *data, T1Scratch *scratch,
                            int32_t *tiles, hipStream_t s, uint32_t *ubuf, uint32_t fixed_words, const DecSeg *segs,
                            const uint32_t *seg_first, uint32_t cblksty, const uint8_t *roi, uint32_t bpw_req) {
    if (!n) return hipSuccess;
    // a call alone on the GPU (bpw_req: the lone packing) or a small one
    // unstuffs a segment per wavefront: 1.37 ms -> 0.27 ms per 8K frame, lone
    // decode T1 29.0 / 29.8 -> 28.1 / 27.5 ms; under 16 frames in flight the
    // lane-per-block pass does the same work in fewer instructions, and the
    // batch is issue-bound: 3529 / 3473 vs 3473 / 3415 Mpixels/s with the
    // wavefront pass (profiles/r05/t1_unstuff_wave_ab.txt)
    if (bpw_req || n <= 4096)
        hipLaunchKernelGGL(k_t1_unstuff_w, dim3((n + 3) / 4), dim3(256), 0, s, blocks, n, data, ubuf, fixed_words, segs,
                           seg_first);
    else
        hipLaunchKernelGGL(k_t1_unstuff, dim3((n + 63) / 64), dim3(64), 0, s, blocks, n, data, ubuf, fixed_words, segs,
                           seg_first);
    const uint32_t bpw = dwt_options().t1_dec_bpw ? (uint32_t)dwt_options().t1_dec_bpw
                         : bpw_req                ? bpw_req
                                                  : t1_blocks_per_wave(n);
    // DEC_WAVES wavefronts per workgroup share the LUTs (roi only for BYPASS:
    // the ROI shift only moves BYPASS pass boundaries)
    const uint32_t nw = (n + bpw - 1) / bpw, nwg = (nw + DEC_WAVES - 1) / DEC_WAVES;
    // A launch of few blocks does not fill the GPU, so occupancy buys nothing
    // and the 128-VGPR cap's spills sit on each lane's chain: single-wavefront
    // workgroups at the uncapped 144 VGPRs -- the 512^2 image (70 blocks)
    // decodes in 9.1-9.4 ms of T1 against 16.8-18.4 (profiles/r05/
    // t1_lone_variants.txt); the 4K frame (6,321 blocks, more than 4,096)
    // and the lone 8K frame were the same either way
    if (n <= 4096) {
        if (cblksty & CBLKSTY_LAZY)
            hipLaunchKernelGGL((k_t1_decode_ub<DEC_LANES, true, 1, 1>), dim3(nw), dim3(DEC_LANES), 0, s, blocks, n,
                               (const uint32_t *)ubuf, fixed_words, scratch, segs, seg_first, cblksty, roi, bpw);
        else
            hipLaunchKernelGGL((k_t1_decode_ub<DEC_LANES, false, 1, 1>), dim3(nw), dim3(DEC_LANES), 0, s, blocks, n,
                               (const uint32_t *)ubuf, fixed_words, scratch, segs, seg_first, cblksty, nullptr, bpw);
    } else if (cblksty & CBLKSTY_LAZY)
        hipLaunchKernelGGL((k_t1_decode_ub<DEC_LANES, true, DEC_WAVES, DEC_WAVES>), dim3(nwg), dim3(DEC_LANES * DEC_WAVES),
                           0, s, blocks, n, (const uint32_t *)ubuf, fixed_words, scratch, segs, seg_first, cblksty, roi,
                           bpw);
    else
        hipLaunchKernelGGL((k_t1_decode_ub<DEC_LANES, false, DEC_WAVES, DEC_WAVES>), dim3(nwg),
                           dim3(DEC_LANES * DEC_WAVES), 0, s, blocks, n, (const uint32_t *)ubuf, fixed_words, scratch,
                           segs, seg_first, cblksty, nullptr, bpw);
    hipLaunchKernelGGL(k_t1_rebuild, dim3((n + 8 * RB_WAVES - 1) / (8 * RB_WAVES), 64 / RB_ROWS), dim3(64 * RB_WAVES), 0,
                       s, blocks, n, scratch, tiles, roi);
    return hipGetLastError();
}

hipError_t launch_gather(const uint8_t *hdr, const uint8_t *slab, const GatherItem *items, uint32_t n, uint8_t *dst,
                         hipStream_t s) {
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(k_gather, dim3(n), dim3(256), 0, s, hdr, slab, items, n, dst);
    return hipGetLastError();
}

}  // namespace grkgpu
