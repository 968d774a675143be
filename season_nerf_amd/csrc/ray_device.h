// A kernel that walks a ray forms its sample points, deltas and PS through this header: one copy of the bit-sensitive ray arithmetic.
// Device-only, stateless, everything __forceinline__: a helper takes values and returns values; what is loaded where, and what lives across an
// MFMA chain, stays the caller's decision.
#pragma once
#include <hip/hip_runtime.h>

namespace snerf {

// the two output non-linearities are no ray arithmetic: they stand here because train_kernels.hip needs them too and does not include mlp_device.h
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }   // torch Softplus(beta 1, thr 20)
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// ---- a ray's samples (misc.py:234-247)
// one coordinate of the sample at t: top (1 - t) + bot t, two rounded products and one add, no fma
__device__ __forceinline__ float ray_coord(float top, float bot, float t) {
    return __fadd_rn(__fmul_rn(top, __fsub_rn(1.f, t)), __fmul_rn(bot, t));
}
__device__ __forceinline__ void ray_point(float tx, float ty, float tz, float bx, float by, float bz, float t, float& x0, float& x1, float& x2) {
    x0 = ray_coord(tx, bx, t);
    x1 = ray_coord(ty, by, t);
    x2 = ray_coord(tz, bz, t);
}
// delta = ||top - bot|| / S (misc.py:243)
__device__ __forceinline__ float ray_delta(float tx, float ty, float tz, float bx, float by, float bz, int S) {
    const float dx = tx - bx, dy = ty - by, dz = tz - bz;
    return __fdiv_rn(__fsqrt_rn(__fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz))), (float)S);
}
// outside [-1, 1]^3 (Eval_Tools_2.py:321-325); a NaN coordinate is inside
__device__ __forceinline__ bool outside_cube(float x, float y, float z) { return x > 1.f || x < -1.f || y > 1.f || y < -1.f || z > 1.f || z < -1.f; }

// ---- wave primitives over the 64 lanes of a wavefront
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_incl_scan(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}
// The exclusive prefix of the same scan: the inclusive value of the lane below, 0 in lane 0.  NOT incl - v: that recovers the prefix from a
// sum which an opaque sample's own v = rho * delta dominates, leaving it with half an ulp of v as its absolute error - and the sample's
// transmittance exp(-prefix), which carries the ray, with that as its relative error ("Transmittance by a shifted scan").
__device__ __forceinline__ float wave_excl_of(float incl, int lane) {
    const float below = __shfl_up(incl, 1, 64);
    return lane == 0 ? 0.f : below;
}
// ---- the same over each 32-lane half of a wavefront; `sl`: the lane within its half
__device__ __forceinline__ float half_incl_scan(float v, int sl) {
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) {
        const float t = __shfl_up(v, o, 32);
        if (sl >= o) v += t;
    }
    return v;
}
__device__ __forceinline__ float half_excl_of(float incl, int sl) {
    const float below = __shfl_up(incl, 1, 32);
    return sl == 0 ? 0.f : below;
}

// ---- one step of the transmittance scan (Eval_Tools_2.py:13-16,187-215): from this lane's y = rho delta (0 where !in) and the optical depth `carry` of
// the steps before, PV = exp(-exclusive prefix), PE = 1 - exp(-y), PS = PV PE (0 where !in), and the optical depth behind the step, which the caller
// stores back (`carry` goes in by value: a local whose address is taken is promoted to a register later than its neighbours, and the kernel's code moves).
struct RayStep {
    float pv, pe, ps, carry;
};
__device__ __forceinline__ RayStep transmit_step(float y, bool in, int lane, float carry) {      // 64 samples a step
    const float incl = wave_incl_scan(y, lane);
    const float excl = carry + wave_excl_of(incl, lane);
    RayStep r;
    r.carry = carry + __shfl(incl, 63, 64);
    r.pv = expf(-excl);
    r.pe = 1.f - expf(-y);
    r.ps = in ? r.pv * r.pe : 0.f;
    return r;
}
__device__ __forceinline__ RayStep transmit_step_half(float y, bool in, int sl, float carry) {   // 32 samples a step, in each half
    const float incl = half_incl_scan(y, sl);
    const float excl = carry + half_excl_of(incl, sl);
    RayStep r;
    r.carry = carry + __shfl(incl, 31, 32);
    r.pv = expf(-excl);
    r.pe = 1.f - expf(-y);
    r.ps = in ? r.pv * r.pe : 0.f;
    return r;
}

// ---- where the ray of image position (row, col) crosses the height h: the 2x2 solve of pre_NeRF/P_Img.py:133-147 `invert_P` on the 3x4 camera P, in float64
__device__ __forceinline__ void invert_P(const double* P, double row, double col, double h, double& x, double& y) {
    const double a11 = P[0] - P[8] * row, a12 = P[1] - P[9] * row, a21 = P[4] - P[8] * col, a22 = P[5] - P[9] * col;
    const double den = a11 * a22 - a12 * a21;
    const double c2 = P[6] * h + P[7] - P[10] * h * col - P[11] * col;     // P23 h + P24 - P33 h y - P34 y
    const double c1 = P[2] * h + P[3] - P[10] * h * row - P[11] * row;     // P13 h + P14 - P33 h x - P34 x
    x = (a12 * c2 - a22 * c1) / den;
    y = (-a11 * c2 + a21 * c1) / den;
}

}  // namespace snerf
