// Device helpers shared by the fused field kernels of all four families (kernels.hip, kernels_ks.hip: bf16 split products; kernels_i8.hip,
// kernels_i8x2.hip: int8 digits): vector types, the LDS-DMA weight ring and its prologue, the exact positional-encoding argument reduction,
// the work of a tile around each family's layer walk (sample position, per-tile inputs, the ray-visibility pass end), output non-linearities.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "program.h"
#include "kernels.h"
#include "ray_device.h"
#if defined(SNERF_ABLATE) && !defined(ABL)
#define ABL 0
#endif

namespace snerf {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(3))) char lds_char;
typedef const __attribute__((address_space(3))) float lds_cfloat;
typedef const __attribute__((address_space(3))) u32x4 lds_cu32x4;
typedef const __attribute__((address_space(3))) f32x4 lds_cf32x4;
typedef const __attribute__((address_space(1))) void glb_void;

#ifndef SNERF_RING_D
#define SNERF_RING_D 7
#endif
constexpr int RING_D = SNERF_RING_D;            // ring slots (one chunk each)
constexpr int DMA_PER_WAVE = kChunkBytes / kFragBytes / 4;   // 1 KiB pieces each wave moves per chunk
constexpr int RING_BYTES = RING_D * kChunkBytes;
constexpr int TILE_PTS = 128;                   // points per workgroup tile (4 waves x 32)

struct Frag {          // B operand of one k-step: 8 bf16 hi + 8 bf16 lo of this lane's point
    u32x4 hi, lo;
};

struct Ring {
    uint32_t rd;       // LDS offset of the slot the NEXT ring_step hands to the consumers
    uint32_t wr;       // LDS offset of the slot the next DMA fills
    uint32_t cur;      // LDS offset of the chunk being consumed
    uint32_t goff;     // byte offset in the (cyclic) global stream of the next chunk to fetch
};

__device__ __forceinline__ float sin2pi(float r) { return __builtin_amdgcn_sinf(r); }   // v_sin_f32: revolutions,
__device__ __forceinline__ float cos2pi(float r) { return __builtin_amdgcn_cosf(r); }   // 1.25e-7 abs err (probe_hw)

// Fetch one 16 KiB chunk: 16 pieces of 1 KiB, wave w moves pieces w, w+4, w+8, w+12 (LDS-DMA: each lane's 16 bytes land
// at M0 + lane*16).  Issued through inline asm on purpose: the __builtin_amdgcn_global_load_lds form is FLAT-encoded
// and makes hipcc (ROCm 7.2) treat every later LDS read as dependent on a "pending flat" access, i.e. it emits
// s_waitcnt lgkmcnt(0) in front of every MFMA instead of counted waits (measured: 685 of 685 waits).  hipcc neither
// counts these loads nor waits for them; ring_step's hand-counted vmcnt does (cdna_hip_programming.md 5.7).
// M0 is written and restored inside the one statement; saddr form: address = sgpr base + lane*16.
__device__ __forceinline__ void dma_chunk(const uint8_t* stream, uint32_t goff, lds_char* lds, uint32_t wr, int wave, int lane) {
    const uint8_t* b0 = stream + goff + wave * kFragBytes;                    // wave-uniform
    const uint32_t dst = (uint32_t)(uintptr_t)(lds + wr + wave * kFragBytes); // wave-uniform LDS byte address
    const uint32_t voff = lane * 16;
    uint32_t keep;
#pragma unroll
    for (int part = 0; part < DMA_PER_WAVE / 4; ++part) {
        const uint8_t* bp = b0 + part * 16 * kFragBytes;
        asm volatile(
            "s_mov_b32 %0, m0\n\t"
            "s_mov_b32 m0, %2\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, %3\n\t"
            "s_add_u32 m0, m0, 0x1000\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, %4\n\t"
            "s_add_u32 m0, m0, 0x1000\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, %5\n\t"
            "s_add_u32 m0, m0, 0x1000\n\t"
            "s_nop 0\n\t"
            "global_load_lds_dwordx4 %1, %6\n\t"
            "s_mov_b32 m0, %0"
            : "=&s"(keep)
            : "v"(voff), "s"(dst + part * 16 * kFragBytes), "s"(bp), "s"(bp + 4 * kFragBytes), "s"(bp + 8 * kFragBytes), "s"(bp + 12 * kFragBytes)
            : "memory", "scc");
    }
}

// Ring `rg` with its prologue issued: D-2 chunks in flight (the refill target trails the consumer by two slots; rg.wr = (D-2)*chunk is,
// at the step that publishes chunk k, the slot of chunk k-2).  A macro, not a function: hipcc simplifies an inlined function's body before
// the kernel's, and a function here (Ring by reference or by value) changed the address arithmetic of the prologue's DMAs.
#define RING_PROLOGUE(rg, D, A, lds, wave, lane)                                                          \
    Ring rg;                                                                                             \
    rg.rd = 0;                                                                                           \
    rg.cur = 0;                                                                                          \
    rg.goff = 0;                                                                                         \
    {                                                                                                    \
        uint32_t wr = 0;                                                                                 \
        _Pragma("unroll") for (int c = 0; c < (D) - 2; ++c) {                                            \
            dma_chunk((A).stream, rg.goff, lds, wr, wave, lane);                                         \
            rg.goff += kChunkBytes;                                                                      \
            if (rg.goff >= (A).stream_bytes) rg.goff = 0;                                                \
            wr += kChunkBytes;                                                                           \
        }                                                                                                \
        rg.wr = wr;                                                                                      \
    }

template <int D = RING_D>
__device__ __forceinline__ uint32_t ring_next(uint32_t off) {
    off += kChunkBytes;
    return off == D * kChunkBytes ? 0u : off;
}

// Hand the next chunk to the consumers and refill the slot released TWO chunks ago.
//  - vmcnt((D-3)*DMA_PER_WAVE): all but the (D-3) youngest chunks this wave fetched have landed => chunk `rd` is complete
//    (counted in DMA instructions of THIS wave; extra older loads/stores only make the wait stricter);
//  - s_barrier: every wave's pieces of chunk `rd` have landed, and every wave has issued the MFMAs that consumed the
//    chunk two steps back (its LDS reads are therefore complete) - so the refill needs no lgkmcnt drain, and the
//    software-pipelined fragment reads of the previous chunk stay in flight across the barrier.
template <int D = RING_D>
__device__ __forceinline__ void ring_step(Ring& rg, const uint8_t* stream, uint32_t stream_bytes, lds_char* lds, int wave, int lane) {
#if defined(SNERF_ABLATE) && (ABL & 4)     // timing-only: no ring at all
    return;
#endif
#if defined(SNERF_ABLATE) && (ABL & 64)    // timing-only: the DMA stream without its rendezvous
    asm volatile("" ::: "memory");
#else
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((D - 3) * DMA_PER_WAVE) : "memory");
#endif
#if !(defined(SNERF_ABLATE) && (ABL & 32)) // timing-only (32): the rendezvous without the DMA stream
    dma_chunk(stream, rg.goff, lds, rg.wr, wave, lane);
#endif
    rg.goff += kChunkBytes;
    if (rg.goff >= stream_bytes) rg.goff = 0;
    rg.cur = rg.rd;
    rg.rd = ring_next<D>(rg.rd);
    rg.wr = ring_next<D>(rg.wr);
}

// Persistent launch of a fused kernel of any family: min(n_tiles, n_cu) workgroups (at least one) of `block` threads with `lds_bytes` of dynamic LDS.
template <class Args>
hipError_t launch_fused(void (*kernel)(Args), int64_t n_tiles, int block, int lds_bytes, const Args& a, int n_cu, hipStream_t st) {
    int grid = (int)(n_tiles < n_cu ? n_tiles : n_cu);
    if (grid < 1) grid = 1;
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), lds_bytes, st, a);
    return hipGetLastError();
}

// sin/cos of k_j * x exactly as the reference evaluates them (misc.py:109,127-131): the fp32 argument is
// 2^j * fl32(fl32(pi/2) * x); it is reduced in fp64 (exact power-of-two scaling, exact fract) before v_sin/v_cos.
struct PeArg {
    double u;   // fl32(fl32(pi/2)*x) / (2*pi), revolutions at j = 0
};
__device__ __forceinline__ PeArg pe_arg(float x) {
    const float a0 = __fmul_rn(x, 1.57079637050628662109375f);
    PeArg r;
    r.u = (double)a0 * 0.15915494309189533576888;
    return r;
}
// the same with the power of two given as its exponent (v_ldexp_f64: exact, and no per-lane table of fp64 scales to keep live)
__device__ __forceinline__ void pe_sincos_exp(const PeArg& a, int e, float& c, float& s) {
    const double r = __builtin_ldexp(a.u, e);
    const float f = (float)(r - __builtin_floor(r));
    c = cos2pi(f);
    s = sin2pi(f);
}
__device__ __forceinline__ void pe_sincos(const PeArg& a, double scale, float& c, float& s) {
    const double r = a.u * scale;                 // exact: scale = 2^j
    const float f = (float)(r - __builtin_floor(r));
    c = cos2pi(f);
    s = sin2pi(f);
}

// ---- the field program's per-tile work around the layer walk (the same in every fused field kernel)
// sample position of field point nc (VARIANTs 0-2): given, or sample nc % S of ray nc / S (misc.py:234-247 fused: top*(1-t) + bot*t,
// two roundings + one add, no fma)
__device__ __forceinline__ void field_point(const MlpArgs& A, int64_t nc, float& x0, float& x1, float& x2) {
    if (A.points) {
        x0 = A.points[nc * 3]; x1 = A.points[nc * 3 + 1]; x2 = A.points[nc * 3 + 2];
    } else {
        const int64_t r = nc / A.n_samples;
        const int s = (int)(nc - r * A.n_samples);
        const float t = A.tvals[s];
        x0 = ray_coord(A.top[r * 3], A.bot[r * 3], t);
        x1 = ray_coord(A.top[r * 3 + 1], A.bot[r * 3 + 1], t);
        x2 = ray_coord(A.top[r * 3 + 2], A.bot[r * 3 + 2], t);
    }
}
// the per-tile inputs of group g: sun direction (VARIANT <= 1), class probabilities (VARIANT 0), zero where the variant has none.
// Every per-tile input is loaded before the MFMA chain: a plain load in the middle of the chain makes hipcc drain the LDS-DMA pipeline with vmcnt(0).
template <int VARIANT>
__device__ __forceinline__ void field_tile_inputs(const MlpArgs& A, int64_t g, float& s0, float& s1, float& s2, float* pcls) {
    s0 = 0.f; s1 = 0.f; s2 = 0.f;
#pragma unroll
    for (int c = 0; c < kMaxClasses; ++c) pcls[c] = 0.f;
    if constexpr (VARIANT <= 1) { s0 = A.sun[g * 3]; s1 = A.sun[g * 3 + 1]; s2 = A.sun[g * 3 + 2]; }
    if constexpr (VARIANT == 0) {
        if (A.classes) {
#pragma unroll
            for (int c = 0; c < kMaxClasses; ++c) if (c < A.n_classes) pcls[c] = A.classes[g * A.n_classes + c];
        }
    }
}

// VARIANT 3 ("ray visibility", Eval_Tools_2.py:255-271 / mg_Img_Eval.py:57-70): the density-only program over the samples of a ray, the
// optical depth sum_{j < S-1} rho_j delta_j kept in a register across the ray's ceil(S / 32) passes, one float out per ray:
// vis = exp(-sum).  A wave owns ray `group * waves + wave`; lane l & 31 of pass p evaluates sample 32 p + (l & 31).
struct RaySum {
    float sum;                      // running optical depth of this lane's samples (lives across the ray's passes)
};
// Which 32 samples the p-th pass of a ray evaluates.  The secondary ray runs from `top` (where it leaves the cube towards the sun, t = 0) to `bot` (the point
// whose visibility is asked for, t = 1); the passes walk it FROM THE POINT OUTWARDS: block ceil(S / 32) - 1 first.  The sum does not care about the order, the
// early-out below does: matter that shadows a point of a real scene is the ground / the building the point sits in, i.e. next to the point, and a ray that
// meets it in its first pass is finished after one evaluation of the network instead of three (ray_flags bit 3 = the old order, sun side first: A/B).
__device__ __forceinline__ int raysum_block(const MlpArgs& A, int p) { return (A.ray_flags & 8) ? p : (A.n_samples + 31) / 32 - 1 - p; }
// sample position of this lane in pass p of a walk (ray_coord: top (1 - t) + bot t).  The ray's end points are re-read every pass (cached loads
// before the MFMA chain) and once more after it for the segment length: nothing of them lives across the chain.
__device__ __forceinline__ void walk_point(const MlpArgs& A, int64_t group, int waves, int wave, int p, int lane, float& x0, float& x1, float& x2) {
    const int64_t ray = group * waves + wave;
    const int64_t r = ray < A.n ? ray : A.n - 1;
    const int s = raysum_block(A, p) * 32 + (lane & 31);
    const float t = A.tvals[s < A.n_samples ? s : A.n_samples - 1];
    x0 = ray_coord(A.top[r * 3], A.bot[r * 3], t);
    x1 = ray_coord(A.top[r * 3 + 1], A.bot[r * 3 + 1], t);
    x2 = ray_coord(A.top[r * 3 + 2], A.bot[r * 3 + 2], t);
}
// the same for the visibility sum, whose first pass clears it
__device__ __forceinline__ void raysum_point(RaySum& q, const MlpArgs& A, int64_t group, int waves, int wave, int p, int lane, float& x0, float& x1, float& x2) {
    if (p == 0) q.sum = 0.f;
    walk_point(A, group, waves, wave, p, lane, x0, x1, x2);
}
// lane-half 0 holds the density row; the last sample never counts (PV at the last sample is the EXCLUSIVE prefix, Eval_Tools_2.py:13-16);
// delta = ||top - bot|| / S (misc.py:243) with the composite kernel's operations
__device__ __forceinline__ void raysum_add(RaySum& q, const MlpArgs& A, int64_t group, int waves, int wave, int p, int lane, float rho_raw, float x0, float x1, float x2) {
    // its own basic block (as the `if (h == 0 && valid)` around the other variants' stores): straight-line code here is scheduled up into the last
    // layer's epilogue, where the softplus / division expansions cost 26 registers of scratch (measured)
    if (lane >= 32) return;
    const int64_t ray = group * waves + wave;
    const int64_t r = ray < A.n ? ray : A.n - 1;
    const float delta = ray_delta(A.top[r * 3], A.top[r * 3 + 1], A.top[r * 3 + 2], A.bot[r * 3], A.bot[r * 3 + 1], A.bot[r * 3 + 2], A.n_samples);
    const int s = raysum_block(A, p) * 32 + (lane & 31);
    {   // the sample position again (the registers that held it during the chain are long gone: fewer values live across it).  It and the cube rule mirror
        // ray_coord / outside_cube (ray_device.h): through either helper the three coordinates' products are scheduled in another order than the parent's
        const float t = A.tvals[s < A.n_samples ? s : A.n_samples - 1], omt = __fsub_rn(1.f, t);
        x0 = __fadd_rn(__fmul_rn(A.top[r * 3], omt), __fmul_rn(A.bot[r * 3], t));
        x1 = __fadd_rn(__fmul_rn(A.top[r * 3 + 1], omt), __fmul_rn(A.bot[r * 3 + 1], t));
        x2 = __fadd_rn(__fmul_rn(A.top[r * 3 + 2], omt), __fmul_rn(A.bot[r * 3 + 2], t));
    }
    const bool oob = x0 > 1.f || x0 < -1.f || x1 > 1.f || x1 < -1.f || x2 > 1.f || x2 < -1.f;
    const bool on = s < A.n_samples - 1 && !((A.ray_flags & 2) && oob);
    q.sum += on ? __fmul_rn(softplus_f(rho_raw), delta) : 0.f;
}
// Early-out (round 6): behind a surface the optical depth only grows, and exp(-18) = 1.5e-8 is below the last bit of a visibility - once EVERY ray of the
// workgroup's group has passed 18, the ray's remaining passes (whole evaluations of the density network) change no result by more than that.  The vote is
// workgroup-wide because the waves share the weight ring: all of them skip the same passes, at a pass boundary, where the cyclic stream stands at its
// start either way.  Consecutive secondary rays start at consecutive samples of one primary ray, so a group saturates together.  `vote`: one LDS float per wave
// (kVoteBytes behind each kernel's LDS image); the store is drained and the barrier passed by all waves before the loads; the next vote is a whole pass later.
constexpr float kSaturatedDepth = 18.f;
// `ray`: the ray this wave walks; `slot` / `n_slots`: this wave's vote word and how many the workgroup casts
__device__ __forceinline__ bool raysum_saturated(const RaySum& q, const MlpArgs& A, int64_t ray, int slot, int n_slots, int lane,
                                                 __attribute__((address_space(3))) float* vote) {
    if (A.ray_flags & 4) return false;                        // A/B switch (SNERF_RAYVIS_NO_EARLY_OUT=1): every pass of every ray
    float v = wave_sum(q.sum);
    if (ray >= A.n) v = 1e30f;                                // a ray past the end never holds the group back
    if (lane == 0) vote[slot] = v;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    bool all = true;
    for (int w = 0; w < n_slots; ++w) all = all && vote[w] > kSaturatedDepth;
    return all;
}
__device__ __forceinline__ void raysum_end(RaySum& q, const MlpArgs& A, int64_t group, int waves, int wave, int lane) {
    float v = wave_sum(q.sum);
    const int64_t ray = group * waves + wave;
    if (lane == 0 && ray < A.n) A.out.vis[ray] = expf(-v);
}
// The end of a pass: add its samples; once the ray is done (its last of `passes`, or a workgroup that voted itself saturated) store its
// visibility (`writer`: this wave stores for its ray), then set `pass` back to 0 and advance the persistent loop's `tile`.  `rays`: rays per
// tile; `ray_wave`: the ray of the tile this wave walks; `slot` / `n_slots`: as raysum_saturated.  A macro for the reason RING_PROLOGUE is
// one: as a function (tile and pass by reference) it changed the code around the vote.
#define RAYSUM_PASS_END(q, A, tile, pass, passes, rays, ray_wave, slot, n_slots, writer, lane, rho_raw, x0, x1, x2, vote)           \
    {                                                                                                                           \
        raysum_add(q, A, tile, rays, ray_wave, pass, lane, rho_raw, x0, x1, x2);                                                \
        if (++pass == (passes) || raysum_saturated(q, A, tile * (rays) + (ray_wave), slot, n_slots, lane, vote)) {              \
            if (writer) raysum_end(q, A, tile, rays, ray_wave, lane);                                                           \
            pass = 0;                                                                                                           \
            tile += gridDim.x;                                                                                                  \
        }                                                                                                                       \
    }

// Ray surface (ray_surface_kernel, ray_surface_ks_kernel): the walk of VARIANT 3 - same density-only stream, ring and vote - with the compositing
// scan of composite_kernel run on each pass's 32 densities, so that a height map needs no [R,S] array at all (Quick_Run.py:37-40,207-226;
// Eval_funcs.py:299-319; mg_run_NeRF.py:188-189).  The transmittance is a prefix: the passes run from the ray's top (t = 0) downwards (raysum_block with
// ray_flags bit 3, which the host always sets), and every one of the S samples counts.  Four floats per lane live across the MFMA chain.
struct RaySurf {
    float carry;                    // optical depth of the samples of the passes walked so far (the same in lanes 0..31, 0 in the others)
    float acc, mt, mi;              // this lane's partial sums of PS, PS t_s and PS s
};
// sample position of this lane in pass p: walk_point's, reached through raysum_point on a dummy sum (calling walk_point directly drops two scalar
// instructions from both ray_surface kernels and renumbers their registers); the first pass of a ray clears its sums
__device__ __forceinline__ void raysurf_point(RaySurf& q, const MlpArgs& A, int64_t group, int waves, int wave, int p, int lane, float& x0, float& x1, float& x2) {
    RaySum unused;
    raysum_point(unused, A, group, waves, wave, p, lane, x0, x1, x2);
    if (p == 0) { q.carry = 0.f; q.acc = 0.f; q.mt = 0.f; q.mi = 0.f; }
}
// The pass's 32 samples into the sums: composite_kernel's y, scan, PV, PE and PS (kernels.hip) over the 32 lanes of half 0.  A basic block of its own and the
// end points and t re-read behind the chain, both for the reasons given in raysum_add.  The exclusive prefix is the inclusive value of the lane below
// (kernels.hip wave_excl_of), never incl - y.
__device__ __forceinline__ void raysurf_add(RaySurf& q, const MlpArgs& A, int64_t group, int waves, int wave, int p, int lane, float rho_raw) {
    if (lane >= 32) return;
    const int64_t ray = group * waves + wave;
    const int64_t r = ray < A.n ? ray : A.n - 1;
    const float tx = A.top[r * 3], ty = A.top[r * 3 + 1], tz = A.top[r * 3 + 2];
    const float bx = A.bot[r * 3], by = A.bot[r * 3 + 1], bz = A.bot[r * 3 + 2];
    float delta = ray_delta(tx, ty, tz, bx, by, bz, A.n_samples);
    const int s = raysum_block(A, p) * 32 + lane;
    const bool in = s < A.n_samples;
    const float t = A.tvals[in ? s : A.n_samples - 1];
    float px, py, pz;
    ray_point(tx, ty, tz, bx, by, bz, t, px, py, pz);
    if ((A.ray_flags & 2) && outside_cube(px, py, pz)) delta = 0.f;
    const float y = in ? softplus_f(rho_raw) * delta : 0.f;
    const RayStep st = transmit_step_half(y, in, lane, q.carry);
    q.carry = st.carry;
    const float ps = st.ps;
    q.acc += ps;
    q.mt += ps * t;
    q.mi += ps * (float)s;
}
// the ray's four numbers {sum PS, sum PS t, sum PS s, optical depth walked}: one 16-byte store by lane 0
__device__ __forceinline__ void raysurf_end(const RaySurf& q, const MlpArgs& A, float* out, int64_t ray, int lane) {
    float acc = q.acc, mt = q.mt, mi = q.mi;     // three wave_sums (ray_device.h) interleaved: as three calls the shuffles are scheduled differently
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        mt += __shfl_xor(mt, o, 64);
        mi += __shfl_xor(mi, o, 64);
    }
    if (lane == 0 && ray < A.n) *reinterpret_cast<f32x4*>(out + ray * 4) = f32x4{acc, mt, mi, q.carry};
}
// The end of a pass, as RAYSUM_PASS_END (a macro for the same reason).  The early-out is the vote of raysum_saturated on the optical depth walked so far:
// lane 0 carries it into the vote's butterfly sum, the other lanes add zero.  Behind depth 18 every further PS is below exp(-18) = 1.5e-8.
#define RAYSURF_PASS_END(q, A, out, tile, pass, passes, rays, ray_wave, slot, n_slots, writer, lane, rho_raw, vote)                 \
    {                                                                                                                           \
        raysurf_add(q, A, tile, rays, ray_wave, pass, lane, rho_raw);                                                           \
        RaySum depth;                                                                                                           \
        depth.sum = lane == 0 ? q.carry : 0.f;                                                                                  \
        if (++pass == (passes) || raysum_saturated(depth, A, tile * (rays) + (ray_wave), slot, n_slots, lane, vote)) {          \
            if (writer) raysurf_end(q, A, out, tile * (rays) + (ray_wave), lane);                                               \
            pass = 0;                                                                                                           \
            tile += gridDim.x;                                                                                                  \
        }                                                                                                                       \
    }

// Shadow walk (shadow_walk_kernel, shadow_walk_ks_kernel): the ray surface's walk through the layers of VARIANT 1 - density head and fc_solar_1..4 -
// with the reference's shadow test in the pass end (T_NeRF_Eval_Utils/mg_Shadow_Eval.py:72-104,134-163): per sample the exact visibility PV (get_PV: the
// exclusive-prefix transmittance along the sun ray, formed as raysurf_add forms it) against the learned one, vis = sigmoid(fc_solar_4).  Seven partial
// sums and the carry live across the MFMA chain; no early-out, since the learned visibility behind a surface is scored like any other.
struct RayShadow {
    float carry;                    // optical depth of the samples of the passes walked so far (the same in lanes 0..31, 0 in the others): slot 7
    float tp, ne, nv;               // this lane's counts of samples with PV > .5 and vis > .5, with PV > .5, with vis > .5 (floats: exact below 2^24)
    float se, ae;                   // sum (PV - vis)^2, sum |PV - vis|
    float psv, acc;                 // sum PS vis, sum PS
};
// sample position of this lane in pass p (walk_point's) and the ray's sun direction; the first pass of a ray clears its sums.  The sun direction is a
// per-tile input: loaded here, before the MFMA chain (field_tile_inputs).
__device__ __forceinline__ void rayshadow_point(RayShadow& q, const MlpArgs& A, const float* sun, int64_t group, int waves, int wave, int p, int lane,
                                                float& x0, float& x1, float& x2, float& s0, float& s1, float& s2) {
    walk_point(A, group, waves, wave, p, lane, x0, x1, x2);
    const int64_t ray = group * waves + wave;
    const int64_t r = ray < A.n ? ray : A.n - 1;
    s0 = sun[r * 3]; s1 = sun[r * 3 + 1]; s2 = sun[r * 3 + 2];
    if (p == 0) { q.carry = 0.f; q.tp = 0.f; q.ne = 0.f; q.nv = 0.f; q.se = 0.f; q.ae = 0.f; q.psv = 0.f; q.acc = 0.f; }
}
// The pass's 32 samples into the sums.  y, the scan, PV, PE and PS are raysurf_add's, operation for operation (acc and carry come out as the ray surface's);
// a basic block of its own and the end points and t re-read behind the chain, for the reasons given in raysum_add.  Padding samples (s >= S) count nowhere.
__device__ __forceinline__ void rayshadow_add(RayShadow& q, const MlpArgs& A, int64_t group, int waves, int wave, int p, int lane, float rho_raw, float sv_raw) {
    if (lane >= 32) return;
    const int64_t ray = group * waves + wave;
    const int64_t r = ray < A.n ? ray : A.n - 1;
    const float tx = A.top[r * 3], ty = A.top[r * 3 + 1], tz = A.top[r * 3 + 2];
    const float bx = A.bot[r * 3], by = A.bot[r * 3 + 1], bz = A.bot[r * 3 + 2];
    float delta = ray_delta(tx, ty, tz, bx, by, bz, A.n_samples);
    const int s = raysum_block(A, p) * 32 + lane;
    const bool in = s < A.n_samples;
    const float t = A.tvals[in ? s : A.n_samples - 1];
    float px, py, pz;
    ray_point(tx, ty, tz, bx, by, bz, t, px, py, pz);
    if ((A.ray_flags & 2) && outside_cube(px, py, pz)) delta = 0.f;
    const float y = in ? softplus_f(rho_raw) * delta : 0.f;
    const RayStep st = transmit_step_half(y, in, lane, q.carry);
    q.carry = st.carry;
    const float pv = st.pv, ps = st.ps;
    const float vis = sigmoid_f(sv_raw);
    const bool ex = in && pv > .5f, es = in && vis > .5f;
    const float d = in ? pv - vis : 0.f;
    q.tp += (ex && es) ? 1.f : 0.f;
    q.ne += ex ? 1.f : 0.f;
    q.nv += es ? 1.f : 0.f;
    q.se += d * d;
    q.ae += fabsf(d);
    q.psv += ps * vis;
    q.acc += ps;
}
// the ray's eight numbers {n(PV > .5 and vis > .5), n(PV > .5), n(vis > .5), sum (PV - vis)^2, sum |PV - vis|, sum PS vis, sum PS, optical depth walked}:
// one 32-byte row, two 16-byte stores by lane 0
__device__ __forceinline__ void rayshadow_end(const RayShadow& q, const MlpArgs& A, float* out, int64_t ray, int lane) {
    float tp = q.tp, ne = q.ne, nv = q.nv, se = q.se, ae = q.ae, psv = q.psv, acc = q.acc;      // seven wave_sums interleaved, as raysurf_end's three
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        tp += __shfl_xor(tp, o, 64);
        ne += __shfl_xor(ne, o, 64);
        nv += __shfl_xor(nv, o, 64);
        se += __shfl_xor(se, o, 64);
        ae += __shfl_xor(ae, o, 64);
        psv += __shfl_xor(psv, o, 64);
        acc += __shfl_xor(acc, o, 64);
    }
    if (lane == 0 && ray < A.n) {
        *reinterpret_cast<f32x4*>(out + ray * 8) = f32x4{tp, ne, nv, se};
        *reinterpret_cast<f32x4*>(out + ray * 8 + 4) = f32x4{ae, psv, acc, q.carry};
    }
}
// The end of a pass, as RAYSURF_PASS_END without its vote: every pass of every ray runs.
#define RAYSHADOW_PASS_END(q, A, out, tile, pass, passes, rays, ray_wave, writer, lane, rho_raw, sv_raw)                            \
    {                                                                                                                           \
        rayshadow_add(q, A, tile, rays, ray_wave, pass, lane, rho_raw, sv_raw);                                                 \
        if (++pass == (passes)) {                                                                                               \
            if (writer) rayshadow_end(q, A, out, tile * (rays) + (ray_wave), lane);                                             \
            pass = 0;                                                                                                           \
            tile += gridDim.x;                                                                                                  \
        }                                                                                                                       \
    }

// Solar audit (solar_audit_kernel, solar_audit_ks_kernel): the reference's comparison of the learned sun visibility with the one the density implies
// (T_NeRF_Eval_Utils/mg_Advanced_Solar.py eval_solar_data on component_render_by_dir(include_exact_solar=True), mg_Img_Eval.py:57-70).  The walk is RaySum's -
// density-only stream, passes from the point outwards, the depth-18 vote - but the rays walked are formed here: a workgroup owns a PRIMARY ray r and walks the
// secondary rays of its samples s = 0 .. S-1, four (W = 512: two) at a time, one per wave (wave pair).  Per sample E = exp(-optical depth) is scored against the
// inputs V = est_vis[r S + s] and PS = ps[r S + s]; the eight sums of a primary ray wait in LDS words behind the vote words, one row per wave, touched by lane 0 of
// that wave alone until the ray ends.  One float per lane lives across the MFMA chain.
struct RayAudit {
    float sum;                      // running optical depth of this lane's samples of the secondary ray (RaySum::sum)
};
constexpr int kAuditLdsFloats = 4 * 8;      // behind the vote words: a row of eight sums per wave
// The secondary ray of sample s of primary ray r (render.py _exact_solar_visibility with sun64, i.e. mg_Img_Eval.py:58-60): bot2 = p = top (1 - t_s) + bot t_s as
// raysum_point forms it, K = (1 - p_z) / (float)sun_z in fp32, top2 = (float)((double)p + (double)K sun) with the product and the sum rounded separately.
__device__ __forceinline__ void rayaudit_ends(const MlpArgs& A, const double* sun, int64_t r, int s, float& t0, float& t1, float& t2, float& b0, float& b1, float& b2) {
    const float t = A.tvals[s];
    b0 = ray_coord(A.top[r * 3], A.bot[r * 3], t);
    b1 = ray_coord(A.top[r * 3 + 1], A.bot[r * 3 + 1], t);
    b2 = ray_coord(A.top[r * 3 + 2], A.bot[r * 3 + 2], t);
    const double K = (double)__fdiv_rn(__fsub_rn(1.f, b2), (float)sun[2]);
    t0 = (float)__dadd_rn((double)b0, __dmul_rn(K, sun[0]));
    t1 = (float)__dadd_rn((double)b1, __dmul_rn(K, sun[1]));
    t2 = (float)__dadd_rn((double)b2, __dmul_rn(K, sun[2]));
}
// sample position of this lane in pass p of the secondary ray of sample `s` (clamped by the caller) of primary ray r: raysum_point on the ends above
__device__ __forceinline__ void rayaudit_point(RayAudit& q, const MlpArgs& A, const double* sun, int64_t r, int s, int p, int lane, float& x0, float& x1, float& x2) {
    float t0, t1, t2, b0, b1, b2;
    rayaudit_ends(A, sun, r, s, t0, t1, t2, b0, b1, b2);
    if (p == 0) q.sum = 0.f;
    const int j = raysum_block(A, p) * 32 + (lane & 31);
    ray_point(t0, t1, t2, b0, b1, b2, A.tvals[j < A.n_samples ? j : A.n_samples - 1], x0, x1, x2);
}
// raysum_add on the ends above, operation for operation (a basic block of its own and everything re-formed behind the chain, for the reasons given there).
// `counts`: false for a wave whose sample index is past the ray's last - it walked a clamped point and adds nothing.
__device__ __forceinline__ void rayaudit_add(RayAudit& q, const MlpArgs& A, const double* sun, int64_t r, int s, bool counts, int p, int lane, float rho_raw) {
    if (lane >= 32) return;
    float t0, t1, t2, b0, b1, b2;
    rayaudit_ends(A, sun, r, s, t0, t1, t2, b0, b1, b2);
    const float delta = ray_delta(t0, t1, t2, b0, b1, b2, A.n_samples);
    const int j = raysum_block(A, p) * 32 + (lane & 31);
    // the point and the cube rule mirror ray_coord / outside_cube (ray_device.h), for the reason given in raysum_add
    const float t = A.tvals[j < A.n_samples ? j : A.n_samples - 1], omt = __fsub_rn(1.f, t);
    const float x0 = __fadd_rn(__fmul_rn(t0, omt), __fmul_rn(b0, t));
    const float x1 = __fadd_rn(__fmul_rn(t1, omt), __fmul_rn(b1, t));
    const float x2 = __fadd_rn(__fmul_rn(t2, omt), __fmul_rn(b2, t));
    const bool oob = x0 > 1.f || x0 < -1.f || x1 > 1.f || x1 < -1.f || x2 > 1.f || x2 < -1.f;
    const bool on = counts && j < A.n_samples - 1 && !((A.ray_flags & 2) && oob);
    q.sum += on ? __fmul_rn(softplus_f(rho_raw), delta) : 0.f;
}
// The end of a secondary ray: E = exp(-sum) by raysum_end's butterfly, stored to exact[i] if asked for, and scored into this wave's row of sums
// {n(E > .5 and V > .5), n(E > .5), n(V > .5), sum E PS, sum V PS, sum PS, sum (E - V)^2, sum |E - V|} by lane 0.  `first`: the ray's first group clears the row.
__device__ __forceinline__ void rayaudit_score(const RayAudit& q, bool counts, bool first, int64_t i, const float* est_vis, const float* ps, float* exact, int lane,
                                               __attribute__((address_space(3))) float* row) {
    float v = wave_sum(q.sum);
    if (lane != 0) return;
    float a[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) a[k] = first ? 0.f : row[k];
    if (counts) {
        const float E = expf(-v), V = est_vis[i], PS = ps[i];
        if (exact) exact[i] = E;
        const bool ex = E > .5f, es = V > .5f;
        const float d = E - V;
        a[0] += (ex && es) ? 1.f : 0.f;
        a[1] += ex ? 1.f : 0.f;
        a[2] += es ? 1.f : 0.f;
        a[3] += E * PS;
        a[4] += V * PS;
        a[5] += PS;
        a[6] += d * d;
        a[7] += fabsf(d);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) row[k] = a[k];
}
// The end of a primary ray: the rows of the `n_rows` scoring waves added in the order of the waves, one 32-byte row stored by lane 0 of wave 0.  Both barriers are
// passed by every wave of the workgroup (the caller's flow is workgroup-uniform, see solar_audit_kernel): the first orders the rows' last stores before the
// loads, the second the loads before the next ray's first group clears the rows.
__device__ __forceinline__ void rayaudit_end(float* out, int64_t r, int wave, int lane, int n_rows, __attribute__((address_space(3))) float* rows) {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    if (wave == 0 && lane == 0) {
        float a[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) a[k] = rows[k];
        for (int w = 1; w < n_rows; ++w)
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] += rows[w * 8 + k];
        *reinterpret_cast<f32x4*>(out + r * 8) = f32x4{a[0], a[1], a[2], a[3]};
        *reinterpret_cast<f32x4*>(out + r * 8 + 4) = f32x4{a[4], a[5], a[6], a[7]};
    }
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
// The end of a pass, as RAYSUM_PASS_END (a macro for the same reason).  `s_wave`: the sample this wave walks (unclamped); `per_group`: secondary rays per group; `rows`: the
// rows of sums, `row`: the one of this wave's secondary ray; `writer`: this wave scores for it.  Once the secondary rays of the group are done (last pass, or the workgroup voted itself
// saturated) they are scored and the next group begins; behind the ray's last group the ray ends and the persistent loop advances.
#define RAYAUDIT_PASS_END(q, A, SA, ray, group, groups, per_group, pass, passes, s_wave, slot, n_slots, writer, wave, lane, rho_raw, vote, rows, row)   \
    {                                                                                                                           \
        const bool counts = (s_wave) < A.n_samples;                                                                             \
        const int s_c = counts ? (s_wave) : A.n_samples - 1;                                                                    \
        rayaudit_add(q, A, SA.sun, ray, s_c, counts, pass, lane, rho_raw);                                                      \
        RaySum depth;                                                                                                           \
        depth.sum = q.sum;                                                                                                      \
        if (++pass == (passes) || raysum_saturated(depth, A, counts ? ray : A.n, slot, n_slots, lane, vote)) {                  \
            if (writer) rayaudit_score(q, counts, group == 0, ray * A.n_samples + s_c, SA.est_vis, SA.ps, SA.exact, lane, row); \
            pass = 0;                                                                                                           \
            if (++group == (groups)) {                                                                                          \
                rayaudit_end(SA.out, ray, wave, lane, per_group, rows);                                                         \
                group = 0;                                                                                                      \
                ray += gridDim.x;                                                                                               \
            }                                                                                                                   \
        }                                                                                                                       \
    }

// Film frame (frame_walk_kernel, frame_walk_ks_kernel): the ray surface's walk through the whole layer list of VARIANT 0 - trunk, head, fc_solar_1..4,
// the colour-adjust branch - with the shading and compositing of the reference's film frames in the pass end (T_NeRF_Eval_Utils/mg_movie_maker.py:108-187):
//   Out_Img = sum_s PS_s (vis_s + (1 - vis_s) sky) col_s,    HM = sum_s PS_s linspace(0, 2, S)[s]
// with the learned visibility applied per sample and one colour per season shown in the frame: only the class vector depends on the time, so up to
// kMaxFrameTimes seasons come from one field pass.  The sun direction, the sky colour, the class vectors and delta are the same for every ray of a launch;
// they wait in LDS (`fin`, staged by the kernel before its first barrier: sun 3 | sky 3 | pad 2 | class vectors kMaxFrameTimes x kMaxClasses, zero filled),
// since a plain load inside the chain drains the LDS-DMA pipeline (field_tile_inputs).  Sixteen floats per lane live across the MFMA chain.
constexpr int kFrameLdsFloats = 8 + kMaxFrameTimes * kMaxClasses;
struct RayFrame {
    float carry;                    // optical depth of the samples of the passes walked so far (the same in lanes 0..31, 0 in the others): slot 14
    float acc, mi, psv;             // this lane's partial sums of PS, PS s and PS vis
    float rgb[3 * kMaxFrameTimes];  // ... of PS shade_c col_k[c] at [3 k + c]
};
// the launch's inputs into LDS, by all 256 threads before the kernel's first barrier
__device__ __forceinline__ void frame_stage_inputs(const FrameWalkArgs& FA, __attribute__((address_space(3))) float* fin) {
    const int i = threadIdx.x, C = FA.m.n_classes;
    if (i < kFrameLdsFloats) {
        float v = 0.f;
        if (i < 3) v = FA.sun[i];
        else if (i < 6) v = FA.sky[i - 3];
        else if (i >= 8) {
            const int k = (i - 8) / kMaxClasses, c = (i - 8) % kMaxClasses;
            if (k < FA.n_times && c < C) v = FA.class_vecs[k * C + c];
        }
        fin[i] = v;
    }
}
// sample position of this lane in pass p: walk_point's, through raysum_point on a dummy sum as in raysurf_point and for its reason; the first pass of a
// ray clears its sums
__device__ __forceinline__ void rayframe_point(RayFrame& q, const MlpArgs& A, int64_t group, int waves, int wave, int p, int lane, float& x0, float& x1, float& x2) {
    RaySum unused;
    raysum_point(unused, A, group, waves, wave, p, lane, x0, x1, x2);
    if (p == 0) {
        q.carry = 0.f; q.acc = 0.f; q.mi = 0.f; q.psv = 0.f;
#pragma unroll
        for (int i = 0; i < 3 * kMaxFrameTimes; ++i) q.rgb[i] = 0.f;
    }
}
// The pass's 32 samples into the sums.  The scan, PV, PE and PS are raysurf_add's, operation for operation, on y = softplus(rho) delta with the frame's one
// delta (the spacing of end-point-inclusive samples; the ray's own length is not used); the colour mixing is store_field_outputs'.  A basic block of its
// own and the end points and t re-read behind the chain, for the reasons given in raysum_add.  Padding samples (s >= S) count nowhere.
__device__ __forceinline__ void rayframe_add(RayFrame& q, const MlpArgs& A, float frame_delta, __attribute__((address_space(3))) const float* fin,
                                             int64_t group, int waves, int wave, int p, int lane, float col_r, float col_g, float col_b, float rho_raw,
                                             float sv_raw, const float* adj) {
    if (lane >= 32) return;
    const int64_t ray = group * waves + wave;
    const int64_t r = ray < A.n ? ray : A.n - 1;
    const float tx = A.top[r * 3], ty = A.top[r * 3 + 1], tz = A.top[r * 3 + 2];
    const float bx = A.bot[r * 3], by = A.bot[r * 3 + 1], bz = A.bot[r * 3 + 2];
    float delta = frame_delta;
    const int s = raysum_block(A, p) * 32 + lane;
    const bool in = s < A.n_samples;
    const float t = A.tvals[in ? s : A.n_samples - 1];
    float px, py, pz;
    ray_point(tx, ty, tz, bx, by, bz, t, px, py, pz);
    if ((A.ray_flags & 2) && outside_cube(px, py, pz)) delta = 0.f;
    const float y = in ? softplus_f(rho_raw) * delta : 0.f;
    const RayStep st = transmit_step_half(y, in, lane, q.carry);
    q.carry = st.carry;
    const float ps = st.ps;
    const float vis = sigmoid_f(sv_raw);
    const float sh0 = ps * (vis + (1.f - vis) * fin[3]), sh1 = ps * (vis + (1.f - vis) * fin[4]), sh2 = ps * (vis + (1.f - vis) * fin[5]);
    q.acc += ps;
    q.mi += ps * (float)s;
    q.psv += ps * vis;
#pragma unroll
    for (int k = 0; k < kMaxFrameTimes; ++k) {      // seasons past n_times mix a zero class vector; their slots are cleared at the ray's end
        float ac0 = 0.f, ac1 = 0.f, ac2 = 0.f;
#pragma unroll
        for (int c = 0; c < kMaxClasses; ++c) {
            if (c < A.n_classes) {
                const float pc = fin[8 + k * kMaxClasses + c];
                ac0 = __fadd_rn(ac0, __fmul_rn(adj[3 * c], pc));
                ac1 = __fadd_rn(ac1, __fmul_rn(adj[3 * c + 1], pc));
                ac2 = __fadd_rn(ac2, __fmul_rn(adj[3 * c + 2], pc));
            }
        }
        q.rgb[3 * k] += sh0 * sigmoid_f(col_r + ac0);
        q.rgb[3 * k + 1] += sh1 * sigmoid_f(col_g + ac1);
        q.rgb[3 * k + 2] += sh2 * sigmoid_f(col_b + ac2);
    }
}
// the ray's sixteen numbers {rgb of season 0, 1, 2, 3 (0 past n_times), sum PS, sum PS s, optical depth walked, sum PS vis}: one 64-byte row, four
// 16-byte stores by lane 0
__device__ __forceinline__ void rayframe_end(const RayFrame& q, const MlpArgs& A, int n_times, float* out, int64_t ray, int lane) {
    float acc = q.acc, mi = q.mi, psv = q.psv, rgb[3 * kMaxFrameTimes];      // fifteen wave_sums interleaved, as raysurf_end's three
#pragma unroll
    for (int i = 0; i < 3 * kMaxFrameTimes; ++i) rgb[i] = q.rgb[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        acc += __shfl_xor(acc, o, 64);
        mi += __shfl_xor(mi, o, 64);
        psv += __shfl_xor(psv, o, 64);
#pragma unroll
        for (int i = 0; i < 3 * kMaxFrameTimes; ++i) rgb[i] += __shfl_xor(rgb[i], o, 64);
    }
#pragma unroll
    for (int i = 0; i < 3 * kMaxFrameTimes; ++i) if (i >= 3 * n_times) rgb[i] = 0.f;
    if (lane == 0 && ray < A.n) {
        static_assert(kMaxFrameTimes == 4, "the row has twelve colour slots");
        float* row = out + ray * 16;
        *reinterpret_cast<f32x4*>(row) = f32x4{rgb[0], rgb[1], rgb[2], rgb[3]};
        *reinterpret_cast<f32x4*>(row + 4) = f32x4{rgb[4], rgb[5], rgb[6], rgb[7]};
        *reinterpret_cast<f32x4*>(row + 8) = f32x4{rgb[8], rgb[9], rgb[10], rgb[11]};
        *reinterpret_cast<f32x4*>(row + 12) = f32x4{acc, mi, q.carry, psv};
    }
}
// The end of a pass, as RAYSURF_PASS_END: the same vote on the optical depth walked so far.  Behind depth 18 every further PS is below exp(-18) = 1.5e-8,
// and shade and colour lie in [0, 1].
#define RAYFRAME_PASS_END(q, A, FA, fin, tile, pass, passes, rays, ray_wave, slot, n_slots, writer, lane, col_r, col_g, col_b, rho_raw, sv_raw, adj, vote) \
    {                                                                                                                           \
        rayframe_add(q, A, (FA).delta, fin, tile, rays, ray_wave, pass, lane, col_r, col_g, col_b, rho_raw, sv_raw, adj);       \
        RaySum depth;                                                                                                           \
        depth.sum = lane == 0 ? q.carry : 0.f;                                                                                  \
        if (++pass == (passes) || raysum_saturated(depth, A, tile * (rays) + (ray_wave), slot, n_slots, lane, vote)) {          \
            if (writer) rayframe_end(q, A, (FA).n_times, (FA).out, tile * (rays) + (ray_wave), lane);                           \
            pass = 0;                                                                                                           \
            tile += gridDim.x;                                                                                                  \
        }                                                                                                                       \
    }

// output non-linearities of the field program (T_NeRF_net_v2.py:91-98) for one point; called by the lanes that hold the head rows
template <int VARIANT>
__device__ __forceinline__ void store_field_outputs(const snerf_field_out_dev& O, int64_t n, int C, float x0, float x1, float x2,
                                                    float col_r, float col_g, float col_b, float rho_raw, float sv_raw,
                                                    const float* adj, const float* pcls) {
    if (O.rho) O.rho[n] = softplus_f(rho_raw);
    if (O.points) { O.points[n * 3] = x0; O.points[n * 3 + 1] = x1; O.points[n * 3 + 2] = x2; }
    if constexpr (VARIANT <= 1) {
        if (O.solar_vis) O.solar_vis[n] = sigmoid_f(sv_raw);
    }
    if constexpr (VARIANT == 0) {
        if (O.col_raw) { O.col_raw[n * 3] = col_r; O.col_raw[n * 3 + 1] = col_g; O.col_raw[n * 3 + 2] = col_b; }
        float ac0 = 0.f, ac1 = 0.f, ac2 = 0.f;
#pragma unroll
        for (int c = 0; c < kMaxClasses; ++c) {
            if (c < C) {
                if (O.adjust) {
                    O.adjust[(n * C + c) * 3] = adj[3 * c];
                    O.adjust[(n * C + c) * 3 + 1] = adj[3 * c + 1];
                    O.adjust[(n * C + c) * 3 + 2] = adj[3 * c + 2];
                }
                const float pc = pcls[c];
                ac0 = __fadd_rn(ac0, __fmul_rn(adj[3 * c], pc));
                ac1 = __fadd_rn(ac1, __fmul_rn(adj[3 * c + 1], pc));
                ac2 = __fadd_rn(ac2, __fmul_rn(adj[3 * c + 2], pc));
            }
        }
        if (O.adjust_col) { O.adjust_col[n * 3] = ac0; O.adjust_col[n * 3 + 1] = ac1; O.adjust_col[n * 3 + 2] = ac2; }
        if (O.col) {
            O.col[n * 3] = sigmoid_f(col_r + ac0);
            O.col[n * 3 + 1] = sigmoid_f(col_g + ac1);
            O.col[n * 3 + 2] = sigmoid_f(col_b + ac2);
        }
    }
}

}  // namespace snerf
