// gfx950 kernel of the per-ray (time / sun) networks at widths 64 and 256: one 32-ray tile per workgroup, every layer's 32-row output
// blocks divided over the four waves.
//
// mlp_kernel<PROG_GROUP> (kernels.hip) gives every wave 32 rays of its own and lets it walk the whole chain alone: 4096 rays are 32 workgroups
// and 504 dependent MFMAs per wave.  Here all four waves of a workgroup hold the SAME 32 rays (ray = lane & 31, as there) and
//   * an output block is computed by exactly one wave, over the whole K, in the k-step order, the three-term product order and with the
//     epilogue of run_layer (mlp_bf16_device.h): every output element sees the floating-point operations it sees there, so the results
//     are bit-identical to mlp_kernel<PROG_GROUP> (tests/test_gpu_group_split.py).  K is never split: that would change the order of the sums;
//   * activations cross the waves through LDS: a wave writes the Frag pair of block b at k-steps 2b, 2b+1 of an activation buffer (hi and lo
//     lane-linear, 1 KiB each: conflict-free b128 accesses), one workgroup barrier, every wave reads all k-steps of its next layer's input;
//   * no wave shares a weight fragment with another, so weights go from the packed stream (pack.cpp, unchanged) straight into registers:
//     16-byte buffer loads at lane * 16, GS_PF pairs ahead of the MFMAs; the first GS_PF pairs of G_T1 and G_T2 are requested at the start of the tile, those of the
//     heads after G_T2's MFMAs, where the registers of G_T2's pairs are free again.  No LDS-DMA, no ring.
//
// Schedule of a tile (two barriers):
//   1. G_T1: NB / 4 blocks per wave (W = 64: one block on waves 0 and 1)           -> buffer 0, barrier
//   2. G_T2: the same division                                                     -> buffer 1, barrier
//   3. wave 0: G_CL, softmax, class store; wave 1: G_K1 and G_K2 in its own registers (the sun branch depends on nothing else), sky stores;
//      waves 2 and 3 go on to the next tile.
// Critical path at W = 256: 12 + 96 + 48 MFMAs.
//
// Why two buffers and two barriers are enough (t = tile of this workgroup, in program order):
//   buffer 0 is written in phase 1 (t+1); its last reads are in phase 2 (t), which every wave has completed (data in registers: the barrier
//   waits for LDS reads) before it arrives at barrier 2 (t), and no wave reaches phase 1 (t+1) before all have arrived there;
//   buffer 1 is written in phase 2 (t+1), behind barrier 1 (t+1), which wave 0 - the only reader in phase 3 (t) - takes after that read.
// Every wave executes both barriers of every tile: they stand at the top level of the tile loop, whose bound is workgroup-uniform.
#include "mlp_bf16_device.h"

namespace snerf {

constexpr int GS_TILE = 32;      // rays per workgroup tile
constexpr int GS_PF = 8;         // weight pairs a wave keeps requested ahead of its MFMAs (8 x 96 MFMA cycles: an L2 round trip)

typedef __attribute__((address_space(3))) u32x4 lds_u32x4;

// Weights and biases are read with buffer loads: the address of one is a descriptor + a scalar offset (which pair) + a lane offset (voff = lane * 16, the
// same register for every load).  Written as pointer arithmetic, base + lane * 16 + pair offset, hipcc forms the 64-bit per-lane base once and keeps one
// 64-bit address per pair live across the tile loop: two registers a load, 284 of them spilled at W = 256.  A read past `bytes` returns zero, never faults.
typedef __amdgpu_buffer_rsrc_t Rsrc;
__device__ __forceinline__ Rsrc make_rsrc(const void* p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);     // raw buffer, 32-bit data format, bounds-checked
}
__device__ __forceinline__ u32x4 load16(Rsrc r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}

// N consecutive weight pairs from byte `base` of the stream -> hi[0..N), lo[0..N).  A layer's run of NP pairs on a wave goes through a ring of
// ring_depth(NP) such slots: the first ring_depth(NP) pairs are requested ahead of the layer, the others inside it (run_blocks).
__host__ __device__ constexpr int ring_depth(int np) { return np < GS_PF ? np : GS_PF; }
template <int N>
__device__ __forceinline__ void request_weights(Rsrc wr, uint32_t base, uint32_t voff, u32x4* hi, u32x4* lo) {
#pragma unroll
    for (int q = 0; q < N; ++q) {
        hi[q] = load16(wr, voff, base + q * kPairBytes);
        lo[q] = load16(wr, voff, base + q * kPairBytes + kFragBytes);
    }
}
// accumulator of block b of the layer whose biases start at float `start`, initialised with them (the values load_bias reads from the LDS copy of the table);
// hoff = 64 bytes per lane-half (+ 128 bytes per block that the caller's b is counted from).  A wave that asks for rows it does not use (phase 3: the class head's
// wave also reads the rows behind G_CL's, waves 2 and 3 read the sun branch's) reads other layers' rows of the same table: in range; past the table a read gives zero.
__device__ __forceinline__ f32x16 request_bias(Rsrc br, int start, int b, uint32_t hoff) {
    f32x16 acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 t = __builtin_bit_cast(f32x4, load16(br, hoff, (start + b * 32) * 4 + q * 16));
        acc[4 * q] = t[0]; acc[4 * q + 1] = t[1]; acc[4 * q + 2] = t[2]; acc[4 * q + 3] = t[3];
    }
    return acc;
}

// NBW consecutive output blocks of a layer on one wave: acc = bias, KS k-steps of the three-term product in order, then run_layer's epilogue
// (SIN: sin, hi/lo split -> out[2i], out[2i+1]; else the raw accumulator of the only block).  Every index is static after unrolling.
// As in run_layer, the epilogue of block b-1 is emitted in slices inside block b's k-steps, and the pair GS_PF k-steps ahead is requested in the
// k-step that frees its registers.  The sched_barrier at the end of a k-step keeps both there: without it hipcc moves each request down to its
// use to save registers, and every k-step waits for a round trip to L2.
template <int NBW, int KS, bool SIN>
__device__ __forceinline__ void run_blocks(Rsrc wr, uint32_t base, uint32_t voff, u32x4* whi, u32x4* wlo, const f32x16* init, const Frag* in, Frag* out, f32x16* raw) {
    constexpr int NP = NBW * KS, D = ring_depth(NP);
    constexpr bool PIPE = KS >= 4;
    f32x16 accs[2];
    EpiTmp et[8];
#pragma unroll
    for (int b = 0; b < NBW; ++b) {
        f32x16 acc = init[b];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int q = b * KS + s;
            const u32x4 a_hi = whi[q % D], a_lo = wlo[q % D];
            if (q + D < NP) {
                whi[q % D] = load16(wr, voff, base + (q + D) * kPairBytes);
                wlo[q % D] = load16(wr, voff, base + (q + D) * kPairBytes + kFragBytes);
            }
            acc = mfma3(a_hi, a_lo, in[s], acc);
            if (SIN && b > 0) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    if (PIPE) {
                        const int sA = 1 + (e * (KS - 4)) / 8;
                        if (s == sA + 2) epi_C(e, et[e], out + 2 * (b - 1));
                        if (s == sA + 1) epi_B(e, et[e], out + 2 * (b - 1));
                        if (s == sA) epi_A(accs[(b - 1) & 1], e, et[e]);
                    } else if (s == 0) {
                        epi_A(accs[(b - 1) & 1], e, et[e]);
                        epi_B(e, et[e], out + 2 * (b - 1));
                        epi_C(e, et[e], out + 2 * (b - 1));
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        accs[b & 1] = acc;
    }
    if constexpr (SIN) {
#pragma unroll
        for (int e = 0; e < 8; ++e) epi_A(accs[(NBW - 1) & 1], e, et[e]);
#pragma unroll
        for (int e = 0; e < 8; ++e) epi_B(e, et[e], out + 2 * (NBW - 1));
#pragma unroll
        for (int e = 0; e < 8; ++e) epi_C(e, et[e], out + 2 * (NBW - 1));
    } else {
        *raw = accs[0];
    }
}

// the Frag pairs of blocks b0 .. b0 + NBW - 1 -> k-steps 2 b0 .. of an activation buffer; all KS k-steps of one back
template <int NBW>
__device__ __forceinline__ void store_act(lds_char* buf, int b0, int lane, const Frag* out) {
#pragma unroll
    for (int f = 0; f < 2 * NBW; ++f) {
        lds_char* p = buf + (2 * b0 + f) * kPairBytes + lane * 16;
        *(lds_u32x4*)p = out[f].hi;
        *(lds_u32x4*)(p + kFragBytes) = out[f].lo;
    }
}
template <int KS>
__device__ __forceinline__ void load_act(lds_char* buf, int lane, Frag* in) {
#pragma unroll
    for (int s = 0; s < KS; ++s) {
        lds_char* p = buf + s * kPairBytes + lane * 16;
        in[s].hi = *(lds_cu32x4*)p;
        in[s].lo = *(lds_cu32x4*)(p + kFragBytes);
    }
}

template <int W>
__global__ __launch_bounds__(256, 1) void mlp_group_split_kernel(const MlpArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int C_MAX = kMaxClasses;
    constexpr int KW = W / 16, NB = W / 32, W4P = pad32(W / 4), KW4 = W4P / 16, NB4 = W4P / 32;
    constexpr int BPW = NB >= 4 ? NB / 4 : 1;       // blocks of G_T1 / G_T2 per active wave
    constexpr int NWV = NB / BPW;                   // waves that own blocks of them (4, or 2 at W = 64)
    constexpr int ACT_BYTES = KW * kPairBytes;      // one activation buffer: KW k-steps of one Frag per lane
    lds_char* buf0 = (lds_char*)smem;
    lds_char* buf1 = buf0 + ACT_BYTES;

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5;
    const int C = A.n_classes;
    const bool owner = NWV == 4 || wave < NWV;
    const int b0 = owner ? wave * BPW : 0;          // first block of this wave in G_T1 / G_T2
    const bool cls = wave == 0;                     // phase 3: this wave runs the class head (wave 1: the sun branch)
    const uint32_t voff = lane * 16, hoff = h * 64;

    // where a layer's pairs and biases start (every layer on a chunk boundary; pair b * KS + s from there)
#define W_AT(L) (uint32_t)(prog_chunk_start(PROG_GROUP, W, C_MAX, L) * kChunkBytes)
#define B_AT(L) prog_bias_start(PROG_GROUP, W, C_MAX, L)
    const Rsrc wr = make_rsrc(A.stream, A.stream_bytes), br = make_rsrc(A.bias, (uint32_t)A.bias_floats * 4);
    constexpr uint32_t w_t1 = W_AT(G_T1), w_t2 = W_AT(G_T2), w_cl = W_AT(G_CL), w_k1 = W_AT(G_K1), w_k2 = W_AT(G_K2);
    // the wave's own blocks of G_T1 / G_T2: their distance from the layer's start goes into the lane offset, so that every scalar offset is a constant
    const uint32_t voff_t1 = voff + b0 * PETIME_KS * kPairBytes, voff_t2 = voff + b0 * KW * kPairBytes;

    const int64_t n_tiles = (A.n + GS_TILE - 1) / GS_TILE;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t n = tile * GS_TILE + (lane & 31);
        const bool valid = n < A.n;
        const int64_t nc = valid ? n : A.n - 1;     // rays past the end: clamped inputs, masked stores

        // ---- the tile's inputs and the first weight pairs and the biases of both hidden layers, requested before the first MFMA
        const float t0 = A.time[nc * 4], t1 = A.time[nc * 4 + 1];
        const float s0 = A.sun[nc * 3], s1 = A.sun[nc * 3 + 1], s2 = A.sun[nc * 3 + 2];
        constexpr int D1 = ring_depth(BPW * PETIME_KS), D2 = ring_depth(BPW * KW);
        u32x4 w1h[D1], w1l[D1], w2h[D2], w2l[D2];
        f32x16 it1[BPW], it2[BPW];
        // (requests are not made conditional on the wave: a register array that is written on one side of a branch only is carried around the tile
        // loop as a whole - hundreds of live registers.  A wave without blocks, or without a head, asks for some other wave's and ignores them.)
        request_weights<D1>(wr, w_t1, voff_t1, w1h, w1l);
        request_weights<D2>(wr, w_t2, voff_t2, w2h, w2l);
#pragma unroll
        for (int i = 0; i < BPW; ++i) {
            it1[i] = request_bias(br, B_AT(G_T1), i, hoff + b0 * 128);
            it2[i] = request_bias(br, B_AT(G_T2), i, hoff + b0 * 128);
        }
        __builtin_amdgcn_sched_barrier(0);

        // ---- phase 1: G_T1 (time encoding -> W)
        if (owner) {
            Frag pt[PETIME_KS];
            make_pe_time(t0, t1, h, pt);
            Frag o[2 * BPW];
            run_blocks<BPW, PETIME_KS, true>(wr, w_t1, voff_t1, w1h, w1l, it1, pt, o, nullptr);
            store_act<BPW>(buf0, b0, lane, o);
        }
        __syncthreads();
        // ---- phase 2: G_T2 (W -> W)
        if (owner) {
            Frag in[KW];
            load_act<KW>(buf0, lane, in);
            Frag o[2 * BPW];
            run_blocks<BPW, KW, true>(wr, w_t2, voff_t2, w2h, w2l, it2, in, o, nullptr);
            store_act<BPW>(buf1, b0, lane, o);
        }
        // ---- the heads' first weight pairs and their biases: requested here, where the registers of G_T2's pairs are free again (earlier, they do not fit beside
        // G_T2's input and ring without parking registers), so that the barrier and the read of the activations hide most of the round trip
        // One set of registers for both heads (a set each would be live on every wave, across the barrier): G_CL's ring on wave 0, all pairs of G_K1 and G_K2 on wave 1
        constexpr int DH = ring_depth(KW), NK1 = NB4 * PESUN_KS;
        static_assert(NK1 + KW4 <= DH, "the sun branch's pairs must fit the class head's ring");
        u32x4 hh[DH], hl[DH];
        f32x16 ih[NB4 + 1];
        // (which head: in the lane offset, as b0 above.  Slot q of the sun branch is pair q of G_K1, then pair q - NK1 of G_K2, which starts on its own chunk;
        // the bias rows of G_K1 and G_K2 follow each other in the table.)
        const uint32_t voff_h1 = voff + (cls ? w_cl : w_k1), voff_h2 = voff + (cls ? w_cl : w_k2 - NK1 * kPairBytes);
        request_weights<NK1>(wr, 0, voff_h1, hh, hl);
        request_weights<DH - NK1>(wr, NK1 * kPairBytes, voff_h2, hh + NK1, hl + NK1);
        static_assert(B_AT(G_K2) == B_AT(G_K1) + 32 * NB4, "G_K2's biases follow G_K1's");
#pragma unroll
        for (int i = 0; i <= NB4; ++i) ih[i] = request_bias(br, 0, i, hoff + 4 * (cls ? B_AT(G_CL) : B_AT(G_K1)));
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        // ---- phase 3: the two heads, one wave each
        if (cls) {
            // class softmax (T_NeRF_net_v2.py:77-78)
            Frag in[KW];
            load_act<KW>(buf1, lane, in);
            f32x16 raw;
            run_blocks<1, KW, false>(wr, w_cl, voff, hh, hl, ih, in, nullptr, &raw);
            if (h == 0 && valid) {
                float m = -3.0e38f;
#pragma unroll
                for (int c = 0; c < C_MAX; ++c) if (c < C) m = fmaxf(m, raw[c]);
                float e[C_MAX], sum = 0.f;
#pragma unroll
                for (int c = 0; c < C_MAX; ++c) { e[c] = c < C ? expf(raw[c] - m) : 0.f; sum += e[c]; }
#pragma unroll
                for (int c = 0; c < C_MAX; ++c) if (c < C && A.g_classes) A.g_classes[n * C + c] = e[c] / sum;
            }
        } else if (wave == 1) {
            // sky colour (G_NeRF.py:110-111): sun encoding -> W/4 -> 3, activations in this wave's registers
            Frag ps[PESUN_KS];
            make_pe_sun(s0, s1, s2, h, ps);
            Frag kA[KW4];
            f32x16 raw;
            run_blocks<NB4, PESUN_KS, true>(wr, w_k1, voff, hh, hl, ih, ps, kA, nullptr);
            run_blocks<1, KW4, false>(wr, w_k2, voff, hh + NK1, hl + NK1, ih + NB4, kA, nullptr, &raw);
            if (h == 0 && valid) {
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    if (A.g_sky_raw) A.g_sky_raw[n * 3 + k] = raw[k];
                    if (A.g_sky) A.g_sky[n * 3 + k] = sigmoid_f(raw[k]);
                }
            }
        }
    }
#undef W_AT
#undef B_AT
}

int mlp_group_split_lds_bytes(int W) { return 2 * (W / 16) * kPairBytes; }

hipError_t launch_mlp_group_split(int W, const MlpArgs& a, int n_cu, hipStream_t st) {
    const int64_t n_tiles = (a.n + GS_TILE - 1) / GS_TILE;
    if (W == 64) return launch_fused(mlp_group_split_kernel<64>, n_tiles, 256, mlp_group_split_lds_bytes(64), a, n_cu, st);
    if (W == 256) return launch_fused(mlp_group_split_kernel<256>, n_tiles, 256, mlp_group_split_lds_bytes(256), a, n_cu, st);
    return hipErrorInvalidValue;
}

}  // namespace snerf
