// Device helpers of the int8-digit fused kernels (kernels_i8.hip: one wave per SIMD; kernels_i8x2.hip: two): digit
// fragments, the three-MFMA digit product, per-row tables, the epilogue arithmetic, the encodings as digit fragments.
#pragma once
#include "mlp_device.h"

namespace snerf {

typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) int i32x16;
typedef __attribute__((ext_vector_type(2))) short i16x2;
typedef const __attribute__((address_space(3))) i32x4 lds_ci32x4;

struct Frag8 {          // B operand of one 32-slot k-step: 16 high digits + 16 low digits of this lane's point
    i32x4 hi, lo;
};
struct Acc8 {           // M = sum T a (weight 2^16), X = sum (T b + L a) (weight 2^8)
    i32x16 M, X;
};
struct Tab8 {           // per-row scale and bias of one 32-row block, accumulator order
    f32x16 sc, bi;
};

// four values in [-1,1] -> their four high digits and four low digits (byte t of each dword = value t)
__device__ __forceinline__ void digits4(float v0, float v1, float v2, float v3, int& hi, int& lo) {
    const uint32_t p0 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pknorm_i16(v0, v1));
    const uint32_t p1 = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pknorm_i16(v2, v3));
    hi = (int)__builtin_amdgcn_perm(p1, p0, 0x07050301u);                 // signed high bytes of the four int16
    lo = (int)(__builtin_amdgcn_perm(p1, p0, 0x06040200u) ^ 0x80808080u); // low bytes - 128 (the +128 lives in the bias)
}
__device__ __forceinline__ void pack16(const float* v, Frag8& f) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        int h, l;
        digits4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3], h, l);
        f.hi[q] = h;
        f.lo[q] = l;
    }
}

__device__ __forceinline__ void mfma_i8x3(const i32x4& aT, const i32x4& aL, const Frag8& b, Acc8& acc) {
    acc.M = __builtin_amdgcn_mfma_i32_32x32x32_i8(aT, b.hi, acc.M, 0, 0, 0);
    acc.X = __builtin_amdgcn_mfma_i32_32x32x32_i8(aT, b.lo, acc.X, 0, 0, 0);
    acc.X = __builtin_amdgcn_mfma_i32_32x32x32_i8(aL, b.hi, acc.X, 0, 0, 0);
}

__device__ __forceinline__ Tab8 load_tab(lds_cfloat* tab_l, int b, int h) {
    lds_cf32x4* tp = (lds_cf32x4*)(tab_l + (b * 2 + h) * 32);
    Tab8 t;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 a = tp[q], c = tp[4 + q];
        t.sc[4 * q] = a[0]; t.sc[4 * q + 1] = a[1]; t.sc[4 * q + 2] = a[2]; t.sc[4 * q + 3] = a[3];
        t.bi[4 * q] = c[0]; t.bi[4 * q + 1] = c[1]; t.bi[4 * q + 2] = c[2]; t.bi[4 * q + 3] = c[3];
    }
    return t;
}

// fp32 weights of the raw coordinates (layers that read an encoding): table [quad][dim 0..2][4 elements] behind the layer's
// scale / bias table (program.h prog_table_start); element i = 4 g + j
struct Raw8 {
    f32x16 w[3];
};
__device__ __forceinline__ Raw8 load_raw(lds_cfloat* raw_l, int b, int h) {
    lds_cf32x4* tp = (lds_cf32x4*)(raw_l + (b * 2 + h) * 48);
    Raw8 r;
#pragma unroll
    for (int g = 0; g < 4; ++g)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const f32x4 t = tp[g * 3 + d];
            r.w[d][4 * g] = t[0]; r.w[d][4 * g + 1] = t[1]; r.w[d][4 * g + 2] = t[2]; r.w[d][4 * g + 3] = t[3];
        }
    return r;
}
__device__ __forceinline__ float add_raw(float z, const Raw8& r, int i, const float* x) {
    return __builtin_fmaf(r.w[0][i], x[0], __builtin_fmaf(r.w[1][i], x[1], __builtin_fmaf(r.w[2][i], x[2], z)));
}

// pre-activation (revolutions for sine layers) of accumulator element i
__device__ __forceinline__ float preact(const Acc8& acc, const Tab8& t, int i) {
    const int m = (int)(((uint32_t)acc.M[i] << 8) + (uint32_t)acc.X[i]);
    return __builtin_fmaf((float)m, t.sc[i], t.bi[i]);
}
// epilogue pieces of a 32x32 block: A(e) = elements 2e, 2e+1 through the sine; Q(g) = digits of elements 4g..4g+3
template <bool RAW = false>
__device__ __forceinline__ void epi_A(const Acc8& acc, const Tab8& t, int e, float* ev, const Raw8* rw = nullptr, const float* rx = nullptr) {
    if constexpr (RAW) {
        ev[2 * e] = sin2pi(add_raw(preact(acc, t, 2 * e), *rw, 2 * e, rx));
        ev[2 * e + 1] = sin2pi(add_raw(preact(acc, t, 2 * e + 1), *rw, 2 * e + 1, rx));
        return;
    }
#if defined(SNERF_ABLATE) && (ABL & 8)      // timing-only: no transcendental; 2 fract(z) - 1 keeps the data as random as sin does
    ev[2 * e] = __builtin_fmaf(__builtin_amdgcn_fractf(preact(acc, t, 2 * e)), 2.f, -1.f);
    ev[2 * e + 1] = __builtin_fmaf(__builtin_amdgcn_fractf(preact(acc, t, 2 * e + 1)), 2.f, -1.f);
#elif defined(SNERF_ABLATE) && (ABL & 16)   // timing-only: no epilogue arithmetic at all but the digit split
    ev[2 * e] = __builtin_bit_cast(float, (acc.X[2 * e] & 0x007fffff) | 0x3f000000) - 0.75f;
    ev[2 * e + 1] = __builtin_bit_cast(float, (acc.X[2 * e + 1] & 0x007fffff) | 0x3f000000) - 0.75f;
#else
    ev[2 * e] = sin2pi(preact(acc, t, 2 * e));
    ev[2 * e + 1] = sin2pi(preact(acc, t, 2 * e + 1));
#endif
}

// PE(pos): 32 values per lane-half (program.h pepos_feature), two k-steps
template <bool OPQ = false>
__device__ __forceinline__ void make_pe_pos8(float x0, float x1, float x2, int h, Frag8* pe) {
    float v[32];
    const float xs[3] = {x0, x1, x2};
    // lane-half h evaluates frequencies 2^(5h) .. 2^(5h+4).  The five exponents are loop-invariant per lane: left alone, hipcc hoists them out of the
    // persistent tile loop and keeps five registers alive across the whole MFMA chain (the ray-visibility variant of the two-wave kernel spilled them);
    // OPQ makes them opaque: recomputed per tile (five v_add per 32 points).  Off for the other variants (their allocation is at its edge as it is).
    int hv = h;
    if constexpr (OPQ) asm volatile("" : "+v"(hv));
    const int e0 = 5 * hv;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const PeArg a = pe_arg(xs[d]);
#pragma unroll
        for (int q = 0; q < 5; ++q) pe_sincos_exp(a, e0 + q, v[10 * d + 2 * q], v[10 * d + 2 * q + 1]);
        __builtin_amdgcn_sched_barrier(0);        // one coordinate's fp64 reductions at a time (register pressure)
    }
    v[30] = h ? x2 : x0;
    v[31] = h ? 0.f : x1;
    pack16(v, pe[0]);
    pack16(v + 16, pe[1]);
}
// PE(sun): 16 values per lane-half (pesun_feature), one k-step
__device__ __forceinline__ void make_pe_sun8(float x0, float x1, float x2, int h, Frag8* pe) {
    float v[16];
    const float xs[3] = {x0, x1, x2};
    const int e0 = 2 * h;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const PeArg a = pe_arg(xs[d]);
#pragma unroll
        for (int q = 0; q < 2; ++q) pe_sincos_exp(a, e0 + q, v[4 * d + 2 * q], v[4 * d + 2 * q + 1]);
    }
    v[12] = h ? x2 : x0;
    v[13] = h ? 0.f : x1;
    v[14] = 0.f;
    v[15] = 0.f;
    pack16(v, pe[0]);
}

// ---- the same digits on v_mfma_i32_16x16x64_i8 (program.h "k64"; kernels_i8x2.hip run_layer16).  Lane l = 16 g + c works for the TWO points c and 16 + c
// of its wave's 32 (column groups 0 and 1) and holds, of each, the 16 k bytes of lane group g.
struct FragK {          // B operand of one 64-slot k-step, per column group: 16 high digits + 16 low digits
    i32x4 hi[2], lo[2];
};
struct AccK {           // M, X as in Acc8: rows 4 g + i of column c, per column group
    i32x4 M[2], X[2];
};
// the digit products of one weight pair: six MFMAs, the two column groups alternating (no MFMA waits for the one issued before it)
__device__ __forceinline__ void mfma_k64x3(const i32x4& aT, const i32x4& aL, const FragK& b, AccK& acc) {
    acc.M[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aT, b.hi[0], acc.M[0], 0, 0, 0);
    acc.M[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aT, b.hi[1], acc.M[1], 0, 0, 0);
    acc.X[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aT, b.lo[0], acc.X[0], 0, 0, 0);
    acc.X[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aT, b.lo[1], acc.X[1], 0, 0, 0);
    acc.X[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aL, b.hi[0], acc.X[0], 0, 0, 0);
    acc.X[1] = __builtin_amdgcn_mfma_i32_16x16x64_i8(aL, b.hi[1], acc.X[1], 0, 0, 0);
}
// the coordinates of this lane's two points from the one-point-per-lane form around the chain (lane l & 31 = point): xq[column group][dim]
__device__ __forceinline__ void k64_two_points(float x0, float x1, float x2, int lane, float (*xq)[3]) {
    asm volatile("" : "+v"(lane));      // the source lanes are formed here, per tile (not hoisted out of the tile loop and kept across the chain)
#pragma unroll
    for (int cg = 0; cg < 2; ++cg) {
        const int src = 16 * cg + (lane & 15);
        xq[cg][0] = __shfl(x0, src, 64); xq[cg][1] = __shfl(x1, src, 64); xq[cg][2] = __shfl(x2, src, 64);
    }
}
// row r of a raw head's block (raw[4 cg + i] = row 4 g + i of point 16 cg + c) as one value per point, in lane l & 31 = point
__device__ __forceinline__ float k64_head_row(const float* raw, int r, int lane) {
    asm volatile("" : "+v"(lane));      // as in k64_two_points
    const int src = 16 * (r / 4) + (lane & 15);
    const float a = __shfl(raw[r % 4], src, 64), b = __shfl(raw[4 + r % 4], src, 64);
    return (lane & 16) ? b : a;
}
// PE(pos): pairs p = 8 g + q (k64_pepos_feature), cos in byte 2 q, sin in 2 q + 1.  The per-lane pair indices are made opaque per tile: left visible, hipcc
// hoists what it derives from them out of the persistent tile loop and keeps it alive across the whole chain.
__device__ __forceinline__ void make_pe_pos_k64(const float (*xq)[3], int g, FragK& pe) {
    int gv = g;
    asm volatile("" : "+v"(gv));
#pragma unroll
    for (int cg = 0; cg < 2; ++cg) {
        float v[16];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int p = 8 * gv + q, d = p / 10, f = p - 10 * d;
            const PeArg a = pe_arg(d == 0 ? xq[cg][0] : d == 1 ? xq[cg][1] : xq[cg][2]);
            pe_sincos_exp(a, f, v[2 * q], v[2 * q + 1]);
            if (q >= 6) {                         // pairs 30, 31 of lane group 3: pads (their weights are zero)
                v[2 * q] = p < 30 ? v[2 * q] : 0.f;
                v[2 * q + 1] = p < 30 ? v[2 * q + 1] : 0.f;
            }
        }
        Frag8 f8;
        pack16(v, f8);
        pe.hi[cg] = f8.hi;
        pe.lo[cg] = f8.lo;
        __builtin_amdgcn_sched_barrier(0);        // one point's fp64 reductions at a time (register pressure)
    }
}
// PE(sun): pairs p = 3 g + q in bytes 0..5 (k64_pesun_feature), the rest pads
__device__ __forceinline__ void make_pe_sun_k64(const float (*sq)[3], int g, FragK& pe) {
    int gv = g;
    asm volatile("" : "+v"(gv));
#pragma unroll
    for (int cg = 0; cg < 2; ++cg) {
        float v[16];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const int p = 3 * gv + q, d = p >> 2, f = p & 3;
            const PeArg a = pe_arg(d == 0 ? sq[cg][0] : d == 1 ? sq[cg][1] : sq[cg][2]);
            pe_sincos_exp(a, f, v[2 * q], v[2 * q + 1]);
        }
#pragma unroll
        for (int e = 6; e < 16; ++e) v[e] = 0.f;
        Frag8 f8;
        pack16(v, f8);
        pe.hi[cg] = f8.hi;
        pe.lo[cg] = f8.lo;
    }
}

// ---- The field network's layer lists of the three int8 kernels (mlp_i8_kernel, and field_tiles2 / field_tiles16 of mlp_i8x2_kernel), written once
// (DESIGN 5.1i).  Macros for the reason FIELD_TRUNK (kernels.hip) is one: a function form changed instructions.  A list line names buffers, program.h
// gives the rest:
//     LAYER(L, IN0, IN1, OUT, RAW, RX, PO, PR, PX)
// L the layer, IN0 / IN1 its input fragments, OUT its digit output or RAW its raw rows (the other is nullptr), RX the raw coordinates of the encoding it
// reads (or nullptr); PO / PR / PX are OUT / RAW / RX of layer L - 1, where a carried last block of that layer is finished (kernels_i8x2.hip Carry; every
// variant runs a prefix of the enum order, so the predecessor of L is L - 1).  Block count, k-steps, sine or raw output, encoding or not, table start and
// the carry's shape are the using kernel's LAYER's to derive from the LayerShape of L and L - 1.  The weight stream cannot branch: a kernel runs these
// lists in the order of its stream, and a change to a list is a change to all three kernels and both streams (FMT_I8, k64).
//   trunk (G_NeRF.py:80-91) and sigma / colour head (G_NeRF.py:93-98): pe -> x1f and raw (rows 0..2 colour, 3 density); hA, hB are scratch.  The statements
//   given after rx_p run behind fc6, the last reader of rx_p
#define I8_TRUNK(LAYER, pe, hA, hB, x1f, raw, rx_p, ...)                                                                                            \
    LAYER(F_FC1, pe, nullptr, hA, nullptr, rx_p, nullptr, nullptr, nullptr);                                                                        \
    LAYER(F_FC2, hA, nullptr, hB, nullptr, nullptr, hA, nullptr, rx_p);                                                                             \
    LAYER(F_FC3, hB, nullptr, hA, nullptr, nullptr, hB, nullptr, nullptr);                                                                          \
    LAYER(F_FC4, hA, nullptr, hB, nullptr, nullptr, hA, nullptr, nullptr);                                                                          \
    LAYER(F_FC5, hB, pe, hA, nullptr, rx_p, hB, nullptr, nullptr);                                                                                  \
    LAYER(F_FC6, hA, nullptr, hB, nullptr, nullptr, hA, nullptr, rx_p);                                                                             \
    __VA_ARGS__                                                                                                                                     \
    LAYER(F_FC7, hB, nullptr, hA, nullptr, nullptr, hB, nullptr, nullptr);                                                                          \
    LAYER(F_FC8, hA, nullptr, hB, nullptr, nullptr, hA, nullptr, nullptr);                                                                          \
    LAYER(F_FC9, hB, nullptr, x1f, nullptr, nullptr, hB, nullptr, nullptr);                                                                         \
    LAYER(F_HEAD, x1f, nullptr, nullptr, raw, nullptr, x1f, nullptr, nullptr)
//   solar visibility branch (G_NeRF.py:100-108): x1f, ps = PE(sun) -> raw row 0; sA, sB are scratch.  The statements given after rx_s run behind
//   fc_solar_1: where the head's block is carried into that layer, its rows are complete there
#define I8_SOLAR(LAYER, x1f, ps, sA, sB, raw, rx_s, ...)                                                                                            \
    LAYER(F_S1, x1f, ps, sA, nullptr, rx_s, nullptr, raw, nullptr);                                                                                 \
    __VA_ARGS__                                                                                                                                     \
    LAYER(F_S2, sA, nullptr, sB, nullptr, nullptr, sA, nullptr, rx_s);                                                                              \
    LAYER(F_S3, sB, nullptr, sA, nullptr, nullptr, sB, nullptr, nullptr);                                                                           \
    LAYER(F_S4, sA, nullptr, nullptr, raw, nullptr, sA, nullptr, nullptr)
//   seasonal colour-adjust branch (T_NeRF_net_v2.py:83-87): x1f -> raw rows 0 .. 3 C_MAX; hA, hB are scratch.  The statements given after raw run behind
//   adjust_layer_1 (fc_solar_4's carried block is complete there)
#define I8_ADJUST(LAYER, x1f, hA, hB, raw, ...)                                                                                                     \
    LAYER(F_A1, x1f, nullptr, hA, nullptr, nullptr, nullptr, raw, nullptr);                                                                         \
    __VA_ARGS__                                                                                                                                     \
    LAYER(F_A2, hA, nullptr, hB, nullptr, nullptr, hA, nullptr, nullptr);                                                                           \
    LAYER(F_A3, hB, nullptr, hA, nullptr, nullptr, hB, nullptr, nullptr);                                                                           \
    LAYER(F_AC, hA, nullptr, nullptr, raw, nullptr, hA, nullptr, nullptr)
// what a LAYER reads from the shape (program.h LayerShape) of its layer
__host__ __device__ constexpr bool layer_sine(const LayerShape& s) { return s.out_kind == OUT_SIN; }
__host__ __device__ constexpr bool layer_reads_raw(const LayerShape& s) { return raw_kind(s) != IN_NONE; }

}  // namespace snerf
