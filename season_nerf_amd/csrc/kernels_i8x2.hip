// gfx950 (MI355X / CDNA4): the int8-digit fused field network with TWO waves per SIMD (widths <= 256).
//
//  mlp_i8x2_kernel<W, VARIANT>   the arithmetic of mlp_i8_kernel (kernels_i8.hip, mlp_i8_device.h), re-shaped so that a wave
//                                needs < 256 registers and eight waves (256 points) share every weight chunk:
//     * one wave alone leaves the matrix pipe idle 45 % of the time (profiles/r2/a_pmc.txt: 57 % of its cycles issue, 27 % are
//       issue stalls, 15 % waits) - the epilogue's VALU work, LDS latency and the per-chunk barrier cannot all hide behind
//       its own MFMAs.  With a partner on the same SIMD the pipe is fed by whichever wave has an MFMA ready;
//     * no software-pipelined epilogue and no accumulator ping-pong (that is what the registers went to): a block is
//       24 MFMAs with the next fragments prefetched, then its epilogue (sine + digit split) in two halves;
//     * ring protocol as in the one-wave kernels (mlp_device.h): one counted vmcnt wait + one workgroup barrier per 16 KiB chunk,
//       now shared by eight waves, so the L2 -> LDS weight traffic per point halves.  Waves 0-3 (which reach every barrier early, see
//       run_layer8x2) move the chunk's sixteen 1 KiB pieces, four each; waves 4-7 only take the barrier (all eight moving two pieces each measured
//       slower: DESIGN 5.1b).
//  Measured (profiles/r2): 0.74 ms against 0.82 ms for the one-wave kernel.  The matrix pipe is busy 59 % of the time: the two
//  waves of a SIMD run in step (the per-chunk barrier re-aligns all eight every block), so the pipe saturates while both are
//  in their MFMA phase and idles while both run epilogues.  Tried against that, each without gain: waves 4-7 taking every
//  barrier half a chunk later in their own stream (a protocol in which barrier m publishes chunk m + 1), s_setprio 2 / 3 for
//  the MFMA phase, fragment prefetch depth 1 / 3, MFMA / VALU interleave pinned inside a k-step (sched_group_barrier),
//  waves 4-7 running their epilogue slices in the odd k-steps and waves 0-3 in the even ones.
//  So the two waves running in step is not what leaves the matrix pipe 40 % idle; the chip holds 1.8 GHz in this kernel.
//  Weight stream, tables, digit formats, accuracy: exactly those of kernels_i8.hip (same packed model, bit-identical results).
//  At W = 256 the kernel runs the same digits on v_mfma_i32_16x16x64_i8 from a stream of its own (run_layer16, field_tiles16 below; program.h "k64"):
//  9 % more cycles at a 15 % higher clock, 0.773 -> 0.716 ms per step (profiles/r13), bit-identical results.  The 32x32x32 code stays for W = 64 and
//  behind SNERF_I8X2_MFMA32=1 (api.cpp field_launch: which stream a launch gets decides the code it runs).
#include <type_traits>

#include "mlp_i8_device.h"

namespace snerf {

constexpr int NW2 = 8;                                      // waves per workgroup: two per SIMD
constexpr int TILE2 = 32 * NW2;                             // 256 points per workgroup tile
constexpr int DMA_WAVES2 = 4, PIECES4 = kChunkBytes / kFragBytes / DMA_WAVES2;      // waves 0-3 move a chunk, four 1 KiB pieces each
constexpr int RING2_D = 7;
constexpr int PFX = 2;                                      // weight-fragment pairs requested ahead of their MFMAs
static_assert(PIECES4 == 4 && kChunkPairs == 8, "dma_chunk4 moves four pieces per loading wave; barrier positions assume 8-pair chunks");

struct Ring2 {
    uint32_t wr;       // LDS offset of the slot the next DMA fills
    uint32_t goff;     // byte offset in the (cyclic) global stream of the next chunk to fetch
    uint32_t cur;      // LDS offset of the chunk this wave is reading
};
__device__ __forceinline__ uint32_t ring2_next(uint32_t off) {
    off += kChunkBytes;
    return off == RING2_D * kChunkBytes ? 0u : off;
}
// wave w (0..3) moves pieces 4w .. 4w+3 of the chunk (see dma_chunk in mlp_device.h for why this is inline asm)
__device__ __forceinline__ void dma_chunk4(const uint8_t* stream, uint32_t goff, lds_char* lds, uint32_t wr, int wave, int lane) {
    const uint8_t* b0 = stream + goff + wave * (4 * kFragBytes);
    const uint32_t dst = (uint32_t)(uintptr_t)(lds + wr + wave * (4 * kFragBytes));
    const uint32_t voff = lane * 16;
    uint32_t keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %3\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %4\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %5\n\t"
        "s_add_u32 m0, m0, 0x400\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, %6\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(voff), "s"(dst), "s"(b0), "s"(b0 + kFragBytes), "s"(b0 + 2 * kFragBytes), "s"(b0 + 3 * kFragBytes)
        : "memory", "scc");
}

// Hand the next chunk to the consumers and refill the slot released two chunks ago (ring_step of mlp_device.h for eight waves).  PHASE 0, the loading
// waves: vmcnt((D-3)*4): all but the (D-3) youngest chunks this wave fetched have landed, and so have the other loading waves' pieces once all have
// passed the barrier => the chunk about to be read is complete.  PHASE 1 only takes the barrier.
template <int PHASE>
__device__ __forceinline__ void ring_step2(Ring2& rg, const uint8_t* stream, uint32_t stream_bytes, lds_char* lds, int wave, int lane) {
#if defined(SNERF_ABLATE) && (ABL & 4)     // timing-only: no ring at all
    return;
#endif
    if (PHASE == 0) {
        asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"((RING2_D - 3) * PIECES4) : "memory");
        dma_chunk4(stream, rg.goff, lds, rg.wr, wave, lane);
    } else {
        asm volatile("s_barrier" ::: "memory");      // the loading waves waited for their pieces before they arrived here
    }
    rg.goff += kChunkBytes;
    if (rg.goff >= stream_bytes) rg.goff = 0;
    rg.wr = ring2_next(rg.wr);
}

// per-row scale and bias of accumulator elements 4g .. 4g+3 of block b (table layout: [16 scales | 16 biases] per block and lane-half)
struct TabQ {
    f32x4 sc, bi;
};
// per-row scale and bias from the layer's table start (block b, lane-half h, quad g)
__device__ __forceinline__ TabQ load_tab_quad(lds_cfloat* tab_l, int b, int h, int g) {
    typedef volatile const __attribute__((address_space(3))) f32x4 lds_vf32x4;      // volatile: see load_tab_quad_h
    lds_vf32x4* tp = (lds_vf32x4*)(tab_l + (b * 2 + h) * 32);
    TabQ t;
    t.sc = tp[g];
    t.bi = tp[4 + g];
    return t;
}
// tab_h: a per-lane base that already points at this lane-half's rows of block 0 (tab_l + 32 h): block b, quad g are then IMMEDIATE offsets
__device__ __forceinline__ TabQ load_tab_quad_h(lds_cfloat* tab_h, int b, int g) {
    // volatile: the table is loop-invariant data, and the optimiser otherwise gathers the loads of whole layers ahead of
    // the chain and parks them in scratch (1.7 KB per lane measured) - they must stay where the epilogue needs them
    typedef volatile const __attribute__((address_space(3))) f32x4 lds_vf32x4;
    lds_vf32x4* tp = (lds_vf32x4*)(tab_h + b * 64);
    TabQ t;
    t.sc = tp[g];
    t.bi = tp[4 + g];
    return t;
}
// A layer's last block handed to the next layer (run_layer8x2): its merged sums wait in m[16], and the receiving layer runs the four
// quads of that block inside its own block 0.  TAB = the producing layer's table start (floats from the table base), NB its block
// count, SIN / RAWL its epilogue.  DEP: the producer's output is the receiver's first input, so block NB - 1 is the B operand of
// k-step NB - 1 of every block of the receiver and all four quads must be complete before that k-step of block 0.
template <int TAB_, int NB_, bool SIN_, bool RAWL_, bool DEP_>
struct Carry {
    static constexpr bool on = true, SIN = SIN_, RAWL = RAWL_, DEP = DEP_;
    static constexpr int TAB = TAB_, NB = NB_;
};
struct NoCarry {
    static constexpr bool on = false, SIN = false, RAWL = false, DEP = false;
    static constexpr int TAB = 0, NB = 1;
};
// a carried block can be taken when the receiver has a k-step in front of the one that reads it
__host__ __device__ constexpr bool carry_fits(int nb, bool dep) { return !dep || nb >= 2; }
// where the carried block's results go: the producer's digit fragments (block NB - 1) or raw floats, and its raw coordinates (RAWL)
struct CarryDst {
    Frag8* out;
    f32x16* raw;
    const float* rawx;
};

// what crosses a layer boundary in registers: the merged sums of the producer's last block (HANDOFF / PEND) and the receiver's first PFX
// weight-fragment pairs, requested by the producer in its last PFX k-steps (PRE_OUT / PRE_IN)
struct Boundary {
    int m[16];
    i32x4 fT[PFX], fL[PFX];
};

// epilogue of elements 4g .. 4g+3 of one block from its merged sums m[]: digits into ob (SIN) or floats into raw
template <bool SIN, bool RAWL>
__device__ __forceinline__ void epi_quad(const int* m, int g, const TabQ& t, const f32x4* rqg, const float* rawx, Frag8* ob, f32x16* raw) {
    float v[4];
#if defined(SNERF_ABLATE) && (ABL & 16)   // timing-only: no epilogue arithmetic at all but the digit split
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __builtin_bit_cast(float, (m[4 * g + j] & 0x007fffff) | 0x3f000000) - 0.75f;
#else
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __builtin_fmaf((float)m[4 * g + j], t.sc[j], t.bi[j]);
    if constexpr (RAWL) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = __builtin_fmaf(rqg[0][j], rawx[0], __builtin_fmaf(rqg[1][j], rawx[1], __builtin_fmaf(rqg[2][j], rawx[2], v[j])));
    }
#endif
    if constexpr (SIN) {
#if defined(SNERF_ABLATE) && (ABL & 8)    // timing-only: no transcendental; 2 fract(z) - 1 keeps the data as random as sin does
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = __builtin_fmaf(__builtin_amdgcn_fractf(v[j]), 2.f, -1.f);
#elif !(defined(SNERF_ABLATE) && (ABL & 16))
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = sin2pi(v[j]);
#endif
        int hi, lo;
        digits4(v[0], v[1], v[2], v[3], hi, lo);
        asm volatile("" : "+v"(hi), "+v"(lo));       // the digits exist HERE (nothing may sink the epilogue towards their first use)
        ob->hi[g] = hi;
        ob->lo[g] = lo;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) (*raw)[4 * g + j] = v[j];
    }
}

// The field chain's boundaries (field_tiles2).  A layer's output is its successor's first input everywhere but behind the two one-block
// raw heads: fc_solar_1 reads x1f, not the colour / density head, and adjust_layer_1 reads x1f, not fc_solar_4.
__host__ __device__ constexpr bool field_feeds_next(int l) { return l != F_HEAD && l != F_S4; }
// every variant runs a prefix of the enum order (program.h field_variant_layers): the layer in front of L in the chain is L - 1, also across the two heads
static_assert(F_S1 == F_HEAD + 1 && F_A1 == F_S4 + 1 && F_FC1 == 0, "the kernels' LAYER macros build the carry of layer L from layer L - 1");
// the last layer of a variant's chain: the tile's outputs are read right behind it
__host__ __device__ constexpr int field_last(int variant) { return variant == 0 ? F_AC : variant == 1 ? F_S4 : F_HEAD; }
// One flag per boundary and instantiation: does layer l hand its last block to the next layer?  Not the last layer of a variant (the tile's
// outputs are read right behind it), and not where a one-block producer feeds k-step 0 (W = 64).  The register file is full
// (256 registers, no scratch: tests/test_isa_guards.py): a boundary that costs an instantiation a register is switched off HERE and
// stays exposed as before.
__host__ __device__ constexpr bool field_carries(int W, int variant, int C, int l) {
    return l != field_last(variant) && carry_fits(prog_layer(PROG_FIELD, W, C, l, FMT_I8).n_out / 32, field_feeds_next(l));
}

// The weight pipeline of a layer (run_layer8x2, run_layer16), in terms of the layer's rg, stream, stream_bytes, lds, wave, lane, PHASE and its fragment
// slots fT, fL.  REQUEST: pair QN of the layer into slot SLOT; the first pair of a chunk takes the ring step.
#if defined(SNERF_ABLATE) && (ABL & 2)     // timing-only: weight fragments stay in registers, no LDS reads
constexpr bool kNoFragReads = true;
#else
constexpr bool kNoFragReads = false;
#endif
#define REQUEST(QN, SLOT)                                                                              \
    do {                                                                                               \
        if ((QN) % kChunkPairs == 0) {                                                                 \
            ring_step2<PHASE>(rg, stream, stream_bytes, lds, wave, lane);                              \
            if ((QN) > 0) rg.cur = ring2_next(rg.cur);                                                 \
        }                                                                                              \
        lds_char* ap_ = lds + rg.cur + ((QN) % kChunkPairs) * kPairBytes + lane * 16;                  \
        if (!kNoFragReads) {                                                                           \
            fT[SLOT] = *(lds_ci32x4*)ap_;                                                              \
            fL[SLOT] = *(lds_ci32x4*)(ap_ + kFragBytes);                                               \
        } else {                                                                                       \
            asm volatile("" : "+v"(fT[SLOT]), "+v"(fL[SLOT]));                                         \
        }                                                                                              \
    } while (0)
// pair J (< PFX) of the NEXT layer, which starts on the next chunk: the weight pipeline runs on across the boundary, so the chunk rendezvous
// and the LDS latency of a layer's first fragments hide behind the last k-steps of the layer before (PRE_OUT there, PRE_IN here)
#define REQUEST_NEXT(J, SLOT)                                                                          \
    do {                                                                                               \
        if ((J) == 0) {                                                                                \
            ring_step2<PHASE>(rg, stream, stream_bytes, lds, wave, lane);                              \
            rg.cur = ring2_next(rg.cur);                                                               \
        }                                                                                              \
        lds_char* ap_ = lds + rg.cur + (J) * kPairBytes + lane * 16;                                   \
        if (!kNoFragReads) {                                                                           \
            fT[SLOT] = *(lds_ci32x4*)ap_;                                                              \
            fL[SLOT] = *(lds_ci32x4*)(ap_ + kFragBytes);                                               \
        } else {                                                                                       \
            asm volatile("" : "+v"(fT[SLOT]), "+v"(fL[SLOT]));                                         \
        }                                                                                              \
    } while (0)

// One fused layer (see run_layer8 in kernels_i8.hip for the arithmetic).  Chunk boundaries of the read sequence are compile-time
// positions; every layer starts on one.  The whole layer is ONE basic block for the compiler (no branch): with branches inside
// it hipcc sinks every block's epilogue to the end of the layer and spills the accumulators meanwhile (measured, 2.4 KB scratch).
//   RAWL: the layer reads an encoding; rawx = its three raw coordinates, added in fp32 (table behind the scale / bias table).
//   PHASE (0 / 1) = the wave group (waves 0-3 / 4-7: waves w and w + 4 share a SIMD).  The matrix pipe is arbitrated by age: left
//   alone, the older wave of a SIMD takes every MFMA slot it wants, reaches the chunk barrier early and waits there for the
//   younger one (in-kernel cycle stamps, DESIGN 5.1b: wave 0 spent 30 % of the launch inside s_barrier, wave 4 3 %).  So the
//   priority alternates per k-step (s_setprio 3 in the k-steps of one's own parity, 0 in the others): wave 0's barrier time
//   drops to 13 %, the kernel gains 2.5 %.  Tried on top without gain: the epilogue slices in the k-steps where a wave yields,
//   biased levels ({0,2} against {1,3}: the younger wave then takes the older one's place), alternating the tie-break per
//   k-step pair / per block (the two waves' barrier times even out, their sum and the kernel time do not change).
//   PEND / HANDOFF: the layer boundary.  Inside a layer the epilogue of block b - 1 hides in block b's k-steps; the last block has no
//   successor in its own layer, and block 0 carries nothing.  With HANDOFF the layer only merges its last block into m[] and returns;
//   the next layer names it as PEND (a Carry) and runs its quads in block 0: before k-step NB_prev - 1 where that block is an
//   operand (Carry::DEP: quad g at k-step g (NB_prev - 1) / 4), over the whole block otherwise.  Same arithmetic, same order per
//   element; only its place in the instruction stream moves.  Without HANDOFF the last epilogue runs exposed behind the block loop.
//   PRE_IN / PRE_OUT: the weight pipeline across the boundary.  A layer alone starts with a chunk rendezvous and the LDS latency of its first
//   PFX fragment pairs in front of its first MFMA, with all eight waves in step.  With PRE_OUT the last PFX k-steps of a layer request the
//   NEXT layer's first pairs (its chunk follows in the ring: same rendezvous, same order, PFX k-steps earlier); that layer (PRE_IN) finds
//   them in bd.fT / bd.fL and starts on an MFMA.
template <int NB, int KS0, int KS1, bool SIN, bool RAWL = false, int PHASE = 0, bool OPQ = false, class PEND = NoCarry, bool HANDOFF = false, bool PRE_IN = false,
          bool PRE_OUT = false>
__device__ __forceinline__ void run_layer8x2(Ring2& rg, const uint8_t* stream, uint32_t stream_bytes, lds_char* lds, lds_cfloat* tab0, lds_cfloat* tab_l,
                                             const Frag8* in0, const Frag8* in1, Frag8* out, f32x16* raw, Boundary& bd, const CarryDst& pd,
                                             int wave, int lane, const float* rawx = nullptr) {
    constexpr int KS = KS0 + KS1, NP = NB * KS;
    constexpr int NBP = PEND::NB;
    static_assert(!PRE_OUT || (NP >= PFX && NP % PFX == 0), "the successor expects its pair j in fragment slot j");
    static_assert(!PRE_IN || NP >= PFX, "the predecessor requested PFX pairs of this layer");
    int (&m)[16] = bd.m;
    i32x4 (&fT)[PFX] = bd.fT;
    i32x4 (&fL)[PFX] = bd.fL;
    static_assert(!PEND::on || carry_fits(NBP, PEND::DEP), "a carried block that is the operand of k-step 0 has no k-step to run in");
    static_assert(!(PEND::on && PEND::DEP) || NBP <= KS0, "Carry::DEP: the producer's output is in0");
    typedef volatile const __attribute__((address_space(3))) f32x4 lds_vf32x4;
    f32x4 rq[4][3];        // raw-coordinate weights of the previous block's quads (RAWL), requested with the table entries
    const int h = lane >> 5;
    // OPQ (the ray-visibility variant): table addresses from ONE opaque per-lane base per layer (this lane-half's rows of block 0), every block / quad an
    // immediate offset from it.  Written as absolute addresses (LDS base + layer start + block + h-term: constants above the 64 KiB reach of a ds_read
    // offset) hipcc gave every table row of THAT variant its own address register and hoisted all of them out of the persistent tile loop - ~25 registers
    // alive across the whole chain, 72-104 bytes of scratch (tests/test_isa_guards.py); the asm makes the base un-hoistable, so it lives for one layer.
    // The other variants compile without scratch as they are and keep their addressing (with the opaque bases the full program spills 116 bytes).
    // With a carried block the one base is the PRODUCER's table (it lies below this layer's: both stay immediate offsets).
    lds_cfloat* ptab_l = tab0 + PEND::TAB;
    lds_cfloat* base_h = (PEND::on ? ptab_l : tab_l) + 32 * h;
    if constexpr (OPQ) asm volatile("" : "+v"(base_h));
    lds_cfloat* raw_l = tab_l + 2 * 32 * NB;
    lds_cfloat* raw_h = raw_l + 48 * h;
    lds_cfloat* praw_l = ptab_l + 2 * 32 * NBP;
    lds_cfloat* praw_h = praw_l + 48 * h;
    if constexpr (OPQ) asm volatile("" : "+v"(raw_h));
    if constexpr (OPQ && PEND::RAWL) asm volatile("" : "+v"(praw_h));
    lds_cfloat* tab_h = base_h + (tab_l - (PEND::on ? ptab_l : tab_l));
    lds_cfloat* ptab_h = base_h;
    auto tabq = [&](int b_, int g_) { return OPQ ? load_tab_quad_h(tab_h, b_, g_) : load_tab_quad(tab_l, b_, h, g_); };
    auto ptabq = [&](int g_) { return OPQ ? load_tab_quad_h(ptab_h, NBP - 1, g_) : load_tab_quad(ptab_l, NBP - 1, h, g_); };
    if constexpr (kNoFragReads) {
#pragma unroll
        for (int q = 0; q < PFX; ++q) { fT[q] = i32x4{lane, 1, 2, 3}; fL[q] = i32x4{4, lane, 6, 7}; }
    }
    if constexpr (!PRE_IN) {
#pragma unroll
        for (int q = 0; q < PFX; ++q) {
            if (q < NP) REQUEST(q, q);
        }
    }
    // Software pipeline: when block b starts, the finished accumulators of block b-1 are merged into m[i] = (M << 8) + X
    // (16 registers instead of 32: no second accumulator set), and their epilogue - a quad of elements per slot - runs
    // inside block b's k-steps (quad g at k-step g KS / 4, its table entries requested at the top of that step).  Each
    // wave's stream is then a uniform mix of MFMA and VALU work, so it does not matter that the two waves of a SIMD run
    // in step: whichever has an MFMA ready feeds the pipe.  Block 0 does the same for the block the previous layer handed over.
    Acc8 acc;
    TabQ tq[4];        // table entries of the previous block's quads: requested one k-step before their slice runs
    auto load_rq = [&](int g, int b_of) {
        if constexpr (RAWL) {
            lds_vf32x4* tp = OPQ ? (lds_vf32x4*)(raw_h + (b_of * 8 + g) * 12) : (lds_vf32x4*)(raw_l + ((b_of * 2 + h) * 4 + g) * 12);
            rq[g][0] = tp[0]; rq[g][1] = tp[1]; rq[g][2] = tp[2];
        }
    };
    auto load_prq = [&](int g) {
        if constexpr (PEND::RAWL) {
            lds_vf32x4* tp = OPQ ? (lds_vf32x4*)(praw_h + ((NBP - 1) * 8 + g) * 12) : (lds_vf32x4*)(praw_l + (((NBP - 1) * 2 + h) * 4 + g) * 12);
            rq[g][0] = tp[0]; rq[g][1] = tp[1]; rq[g][2] = tp[2];
        }
    };
    auto quad = [&](int g, int b_of, const TabQ& t) { epi_quad<SIN, RAWL>(m, g, t, rq[g], rawx, out + b_of, raw); };
    auto pquad = [&](int g, const TabQ& t) { epi_quad<PEND::SIN, PEND::RAWL>(m, g, t, rq[g], pd.rawx, pd.out + (NBP - 1), pd.raw); };
    // k-step of a block in which quad g of the block before runs; the carried block where it is an operand: before k-step NBP - 1
    auto slot = [](int g, bool carried) constexpr { return carried && PEND::DEP ? (g * (NBP - 1)) / 4 : (g * KS) / 4; };
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const bool carried = b == 0;
        if (b > 0 || PEND::on) {
            if (b > 0) {
                tq[0] = tabq(b - 1, 0);
                load_rq(0, b - 1);
#pragma unroll
                for (int i = 0; i < 16; ++i) m[i] = (int)(((uint32_t)acc.M[i] << 8) + (uint32_t)acc.X[i]);
            } else {
                tq[0] = ptabq(0);
                load_prq(0);
            }
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) { acc.M[i] = 0; acc.X[i] = 0; }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int q = b * KS + s;
            const i32x4 aT = fT[q % PFX], aL = fL[q % PFX];
            // own parity: this wave's MFMAs first (it runs no epilogue slice in this k-step); else yield to the partner
            if (((s + PHASE) & 1) == 0) __builtin_amdgcn_s_setprio(0); else __builtin_amdgcn_s_setprio(3);
            if (q + PFX < NP) REQUEST(q + PFX, q % PFX);
            else if constexpr (PRE_OUT) REQUEST_NEXT(q + PFX - NP, q % PFX);
            if (b > 0 || PEND::on) {
#pragma unroll
                for (int g = 1; g < 4; ++g) {
                    const int sg = slot(g, carried), lg = sg > 0 ? sg - 1 : 0;
                    if (lg == s) {
                        if (b > 0) { tq[g] = tabq(b - 1, g); load_rq(g, b - 1); }
                        else { tq[g] = ptabq(g); load_prq(g); }
                    }
                }
            }
            mfma_i8x3(aT, aL, s < KS0 ? in0[s] : in1[s - KS0], acc);
            if (b > 0 || PEND::on) {
#pragma unroll
                for (int g = 0; g < 4; ++g)
                    if (slot(g, carried) == s) {
                        if (b > 0) quad(g, b - 1, tq[g]);
                        else pquad(g, tq[g]);
                    }
            }
            asm volatile("" ::: "memory");          // table loads stay in their k-step (the optimiser would gather them up front)
            __builtin_amdgcn_sched_barrier(0);      // ... and so do requests, MFMAs and epilogue slices (register pressure)
        }
    }
    // the last block of the layer: handed to the next layer, or (nothing to hide its epilogue behind but the partner wave) finished here
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = (int)(((uint32_t)acc.M[i] << 8) + (uint32_t)acc.X[i]);
    if constexpr (HANDOFF) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    } else {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            asm volatile("" ::: "memory");
            const TabQ t = tabq(NB - 1, g);
            load_rq(g, NB - 1);
            quad(g, NB - 1, t);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (!PRE_OUT) rg.cur = ring2_next(rg.cur);          // the next layer starts on the next chunk
}

// ---- the same layer on v_mfma_i32_16x16x64_i8 (program.h "k64", mlp_i8_device.h FragK): where the chip holds its clock down, the clock depends on the
// MFMA shape.  Same output tile per wave - 32 points, as two 16-point column groups - and the same ring, chunks and pair size: a weight
// pair read from LDS feeds 3 products x 2 column groups = 6 MFMAs, so the LDS weight bytes per MAC are those of run_layer8x2.
//   * a block is 16 rows x 32 points: accumulators M, X of 2 x 4 registers each, merged into m[8] (m[4 cg + i] = row 4 g + i of point 16 cg + c);
//   * its epilogue is two quads - one per column group, same rows, so ONE table entry (and one set of raw-coordinate weights) per block, requested with
//     the merge - and rides in the next block's k-steps 0 and KS / 2; four blocks fill one k-step of the next layer (out[b / 4], dword b % 4);
//   * PEND / HANDOFF / PRE_IN / PRE_OUT, the s_setprio alternation per k-step and the compiler constraints are those of run_layer8x2.  A carried block that
//     is an operand (Carry::DEP) is dword 3 of the receiver's k-step (NBP - 1) / 4: both quads run before it.
// Per element the arithmetic is epi_quad's, on the same integers: results are bit-identical to run_layer8x2's.
struct BoundaryK {
    int m[8];
    i32x4 fT[PFX], fL[PFX];
};
struct CarryDstK {
    FragK* out;
    float* raw;            // [8]
    const float (*rawx)[3];   // [column group][dim]
};
__host__ __device__ constexpr bool carry_fits_k64(int nb, bool dep) { return !dep || nb >= 5; }
__host__ __device__ constexpr bool field_carries_k64(int W, int variant, int C, int l) {
    return l != field_last(variant) && carry_fits_k64(k64_blocks(k64_layer(W, C, l)), field_feeds_next(l));
}
// quad cg of a block from its merged sums: epi_quad on m[4 cg ..], the digits into dword `dw` of the k-step fragment `ob`
template <bool SIN, bool RAWL>
__device__ __forceinline__ void epi_quad_k64(const int* m, int cg, const TabQ& t, const f32x4* rq, const float (*rawx)[3], FragK* ob, int dw, float* raw) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = __builtin_fmaf((float)m[4 * cg + j], t.sc[j], t.bi[j]);
    if constexpr (RAWL) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = __builtin_fmaf(rq[0][j], rawx[cg][0], __builtin_fmaf(rq[1][j], rawx[cg][1], __builtin_fmaf(rq[2][j], rawx[cg][2], v[j])));
    }
    if constexpr (SIN) {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = sin2pi(v[j]);
        int hi, lo;
        digits4(v[0], v[1], v[2], v[3], hi, lo);
        asm volatile("" : "+v"(hi), "+v"(lo));       // the digits exist HERE
        ob->hi[cg][dw] = hi;
        ob->lo[cg][dw] = lo;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) raw[4 * cg + j] = v[j];
    }
}

template <int NB, int KS0, int KS1, bool SIN, bool RAWL = false, int PHASE = 0, class PEND = NoCarry, bool HANDOFF = false, bool PRE_IN = false,
          bool PRE_OUT = false>
__device__ __forceinline__ void run_layer16(Ring2& rg, const uint8_t* stream, uint32_t stream_bytes, lds_char* lds, lds_cfloat* tab0, lds_cfloat* tab_l,
                                            const FragK* in0, const FragK* in1, FragK* out, float* raw, BoundaryK& bd, const CarryDstK& pd,
                                            int wave, int lane, const float (*rawx)[3] = nullptr) {
    constexpr int KS = KS0 + KS1, NP = NB * KS;
    constexpr int NBP = PEND::NB;
    static_assert(!PRE_OUT || (NP >= PFX && NP % PFX == 0), "the successor expects its pair j in fragment slot j");
    static_assert(!PRE_IN || NP >= PFX, "the predecessor requested PFX pairs of this layer");
    static_assert(!PEND::on || carry_fits_k64(NBP, PEND::DEP), "a carried block that is an operand of k-step 0 has no k-step to run in");
    static_assert(!(PEND::on && PEND::DEP) || NBP == 4 * KS0, "Carry::DEP: the producer's output is in0");
    int (&m)[8] = bd.m;
    i32x4 (&fT)[PFX] = bd.fT;
    i32x4 (&fL)[PFX] = bd.fL;
    typedef volatile const __attribute__((address_space(3))) f32x4 lds_vf32x4;      // volatile: see load_tab_quad_h
    // table addresses: one per-lane base per layer (this lane group's rows of block 0 of the lower of the two tables read here), every block an immediate
    // offset from it.  The lane group is made opaque per layer: every layer's base is a loop invariant of the persistent tile loop, and left visible hipcc
    // computes all of them in front of the loop and keeps them alive across the whole chain (35 registers measured, the allocation spilled).
    int g = lane >> 4;
    asm volatile("" : "+v"(g));
    lds_cfloat* ptab_l = tab0 + PEND::TAB;
    lds_cfloat* lo_l = PEND::on ? ptab_l : tab_l;
    lds_cfloat* base_g = lo_l + 8 * g;
    lds_cfloat* rbase_g = lo_l + 12 * g;
    const int d_own = (int)(tab_l - lo_l);
    auto tabq = [&](int b_) {
        lds_vf32x4* tp = (lds_vf32x4*)(base_g + d_own + b_ * 32);
        TabQ t;
        t.sc = tp[0];
        t.bi = tp[1];
        return t;
    };
    auto ptabq = [&]() {
        lds_vf32x4* tp = (lds_vf32x4*)(base_g + (NBP - 1) * 32);
        TabQ t;
        t.sc = tp[0];
        t.bi = tp[1];
        return t;
    };
    f32x4 rq[3];           // raw-coordinate weights of the previous block's rows (RAWL), requested with its table entry
    auto load_rq = [&](int b_of) {
        if constexpr (RAWL) {
            lds_vf32x4* tp = (lds_vf32x4*)(rbase_g + d_own + 2 * 16 * NB + b_of * 48);
            rq[0] = tp[0]; rq[1] = tp[1]; rq[2] = tp[2];
        }
    };
    auto load_prq = [&]() {
        if constexpr (PEND::RAWL) {
            lds_vf32x4* tp = (lds_vf32x4*)(rbase_g + 2 * 16 * NBP + (NBP - 1) * 48);
            rq[0] = tp[0]; rq[1] = tp[1]; rq[2] = tp[2];
        }
    };
    if constexpr (kNoFragReads) {
#pragma unroll
        for (int q = 0; q < PFX; ++q) { fT[q] = i32x4{lane, 1, 2, 3}; fL[q] = i32x4{4, lane, 6, 7}; }
    }
    if constexpr (!PRE_IN) {
#pragma unroll
        for (int q = 0; q < PFX; ++q) {
            if (q < NP) REQUEST(q, q);
        }
    }
    AccK acc;
    TabQ tq;               // table entry of the previous block (both quads: a block's two column groups are the same rows)
    auto quad = [&](int cg, int b_of) { epi_quad_k64<SIN, RAWL>(m, cg, tq, rq, rawx, out + b_of / 4, b_of % 4, raw); };
    auto pquad = [&](int cg) { epi_quad_k64<PEND::SIN, PEND::RAWL>(m, cg, tq, rq, pd.rawx, pd.out + (NBP - 1) / 4, (NBP - 1) % 4, pd.raw); };
    // k-step of a block in which quad cg of the block before runs; the carried block where it is an operand: before k-step (NBP - 1) / 4
    auto slot = [](int cg, bool carried) constexpr { return carried && PEND::DEP ? (cg * ((NBP - 1) / 4) * 2) / 3 : (cg * KS) / 2; };
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const bool carried = b == 0;
        if (b > 0 || PEND::on) {
            if (b > 0) {
                tq = tabq(b - 1);
                load_rq(b - 1);
#pragma unroll
                for (int i = 0; i < 8; ++i) m[i] = (int)(((uint32_t)acc.M[i >> 2][i & 3] << 8) + (uint32_t)acc.X[i >> 2][i & 3]);
            } else {
                tq = ptabq();
                load_prq();
            }
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int cg = 0; cg < 2; ++cg)
#pragma unroll
            for (int i = 0; i < 4; ++i) { acc.M[cg][i] = 0; acc.X[cg][i] = 0; }
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int q = b * KS + s;
            const i32x4 aT = fT[q % PFX], aL = fL[q % PFX];
            if (((s + PHASE) & 1) == 0) __builtin_amdgcn_s_setprio(0); else __builtin_amdgcn_s_setprio(3);
            if (q + PFX < NP) REQUEST(q + PFX, q % PFX);
            else if constexpr (PRE_OUT) REQUEST_NEXT(q + PFX - NP, q % PFX);
            mfma_k64x3(aT, aL, s < KS0 ? in0[s] : in1[s - KS0], acc);
            if (b > 0 || PEND::on) {
#pragma unroll
                for (int cg = 0; cg < 2; ++cg)
                    if (slot(cg, carried) == s) {
                        if (b > 0) quad(cg, b - 1);
                        else pquad(cg);
                    }
            }
            asm volatile("" ::: "memory");          // table loads stay in their k-step
            __builtin_amdgcn_sched_barrier(0);      // ... and so do requests, MFMAs and epilogue slices (register pressure)
        }
    }
    // the last block of the layer: handed to the next layer, or finished here
#pragma unroll
    for (int i = 0; i < 8; ++i) m[i] = (int)(((uint32_t)acc.M[i >> 2][i & 3] << 8) + (uint32_t)acc.X[i >> 2][i & 3]);
    if constexpr (HANDOFF) {
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    } else {
        asm volatile("" ::: "memory");
        tq = tabq(NB - 1);
        load_rq(NB - 1);
#pragma unroll
        for (int cg = 0; cg < 2; ++cg) {
            quad(cg, NB - 1);
            asm volatile("" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (!PRE_OUT) rg.cur = ring2_next(rg.cur);          // the next layer starts on the next chunk
}
#undef REQUEST
#undef REQUEST_NEXT

// instances built on the 16x16x64 shape (the others, and every instance under SNERF_I8X2_MFMA32=1, run the 32x32x32 code above)
__host__ __device__ constexpr bool k64_built(int W) { return W == 256; }      // all four variants (profiles/r13)
bool i8x2_k64_built(int W, int variant) { return variant >= 0 && variant <= 3 && k64_built(W); }

template <int W, int VARIANT, int PHASE>
__device__ __forceinline__ void field_tiles2(const MlpArgs& A, Ring2& rg, lds_char* lds, __attribute__((address_space(3))) float* tab_lds,
                                             int wave, int lane);
template <int W, int VARIANT, int PHASE>
__device__ __forceinline__ void field_tiles16(const MlpArgs& A, Ring2& rg, lds_char* lds, __attribute__((address_space(3))) float* tab_lds,
                                              int wave, int lane);

template <int W, int VARIANT>
__global__ __launch_bounds__(64 * NW2, 1) void mlp_i8x2_kernel(const MlpArgs A) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int C_MAX = kMaxClasses;
    constexpr int W2 = W / 2;
    lds_char* lds = (lds_char*)smem;
    __attribute__((address_space(3))) float* tab_lds = (__attribute__((address_space(3))) float*)(lds + RING2_D * kChunkBytes);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int h = lane >> 5;
    const int C = A.n_classes;

    for (int i = threadIdx.x; i < A.bias_floats; i += 64 * NW2) tab_lds[i] = A.bias[i];

    Ring2 rg;
    rg.cur = 0;
    rg.goff = 0;
    {
        uint32_t wr = 0;
#pragma unroll
        for (int c = 0; c < RING2_D - 2; ++c) {
            if (wave < DMA_WAVES2) dma_chunk4(A.stream, rg.goff, lds, wr, wave, lane);
            rg.goff += kChunkBytes;
            if (rg.goff >= A.stream_bytes) rg.goff = 0;
            wr += kChunkBytes;
        }
        rg.wr = wr;
    }
    __syncthreads();   // table visible (drains the prologue DMAs once; harmless)

    // the MFMA shape: by width at compile time (k64_built), and there by the stream the host handed over (A.k64: api.cpp field_launch)
    bool k64 = false;
    if constexpr (k64_built(W)) k64 = A.k64 != 0;
    if (k64) {
        if constexpr (k64_built(W)) {
            if (wave < 4) field_tiles16<W, VARIANT, 0>(A, rg, lds, tab_lds, wave, lane);
            else field_tiles16<W, VARIANT, 1>(A, rg, lds, tab_lds, wave, lane);
        }
    } else {
        if (wave < 4) field_tiles2<W, VARIANT, 0>(A, rg, lds, tab_lds, wave, lane);
        else field_tiles2<W, VARIANT, 1>(A, rg, lds, tab_lds, wave, lane);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no LDS-DMA may outlive the workgroup
}

// the tile loop of field_tiles2 on the 16x16x64 shape.  Around the chain a lane keeps field_tiles2's form (lane l & 31 = point: inputs, outputs, the ray sum
// of VARIANT 3 are its code); inside, lane 16 g + c works for points c and 16 + c (mlp_i8_device.h): the coordinates go in and the raw heads' rows come
// out through a few cross-lane reads per tile.
template <int W, int VARIANT, int PHASE>
__device__ __forceinline__ void field_tiles16(const MlpArgs& A, Ring2& rg, lds_char* lds, __attribute__((address_space(3))) float* tab_lds,
                                              int wave, int lane) {
    constexpr int C_MAX = kMaxClasses;
    constexpr int W2 = W / 2;
    const int h = lane >> 5, gq = lane >> 4;
    const int C = A.n_classes;
    const int64_t n_tiles = field_tiles(A.n, VARIANT, TILE2, NW2);
    const int passes = VARIANT == 3 ? (A.n_samples + 31) / 32 : 1;
    int pass = 0;
    RaySum rs;
    for (int64_t tile = blockIdx.x; tile < n_tiles;) {
        const int64_t n = tile * TILE2 + wave * 32 + (lane & 31);
        const bool valid = n < A.n;
        const int64_t nc = valid ? n : A.n - 1;
        const int64_t g = VARIANT == 3 ? 0 : nc / A.group_size;

        float x0, x1, x2;
        if constexpr (VARIANT == 3) raysum_point(rs, A, tile, NW2, wave, pass, lane, x0, x1, x2);
        else field_point(A, nc, x0, x1, x2);
        float s0, s1, s2, pcls[C_MAX];
        field_tile_inputs<VARIANT>(A, g, s0, s1, s2, pcls);
        float rx_p[2][3], rx_s[2][3];      // raw coordinates of this lane's two points: fp32, no digit range
        k64_two_points(x0, x1, x2, lane, rx_p);
        FragK pe;
        make_pe_pos_k64(rx_p, gq, pe);

        constexpr int KW = W / 64, KW2 = W2 / 64;
        FragK hA[KW], hB[KW];
        float raw[8];
        BoundaryK bd;
        // The lists of mlp_i8_device.h.  Everything a line does not name comes from the k64 shape of its layer; the carry a layer receives from that
        // of layer L - 1: HAND(L) = layer L hands its last block to its successor (one flag per boundary, read by both sides).
#define SHAPE(L) k64_layer(W, C_MAX, L)
#define TAB(L) k64_table_start(W, C_MAX, L)
#define HAND(L) (L >= F_FC1 && field_carries_k64(W, VARIANT, C_MAX, L))
#define PEND_T(P) std::conditional_t<HAND(P), Carry<TAB(P), k64_blocks(SHAPE(P)), layer_sine(SHAPE(P)), layer_reads_raw(SHAPE(P)), field_feeds_next(P)>, NoCarry>
#define LAYER(L, IN0, IN1, OUT, RAW, RX, PO, PR, PX)                                                                                                 \
    run_layer16<k64_blocks(SHAPE(L)), SHAPE(L).ks0, SHAPE(L).ks1, layer_sine(SHAPE(L)), layer_reads_raw(SHAPE(L)), PHASE, PEND_T(L - 1), HAND(L),   \
                L != F_FC1, L != field_last(VARIANT)>(rg, A.stream, A.stream_bytes, lds, tab_lds, tab_lds + TAB(L), IN0, IN1, OUT, RAW, bd,         \
                                                      (CarryDstK{PO, PR, PX}), wave, lane, RX)
        FragK x1f[KW2];
        I8_TRUNK(LAYER, &pe, hA, hB, x1f, raw, rx_p,
                 // the lane's own point (l & 31) is one of its two: from here on its coordinates (for the stores) replace the pair's, whose last reader was fc6
                 if constexpr (VARIANT != 3) {
                     const bool up = (lane & 16) != 0;
                     x0 = up ? rx_p[1][0] : rx_p[0][0]; x1 = up ? rx_p[1][1] : rx_p[0][1]; x2 = up ? rx_p[1][2] : rx_p[0][2];
                 });
        // the head's rows 0..2 colour, 3 density (lane group 0); with the solar branch behind it the block finishes inside fc_solar_1
        float col_r, col_g, col_b, rho_raw;
        float sv_raw = 0.f;
        float adj[3 * C_MAX];
#pragma unroll
        for (int i = 0; i < 3 * C_MAX; ++i) adj[i] = 0.f;
#define HEAD_OUT() col_r = k64_head_row(raw, 0, lane), col_g = k64_head_row(raw, 1, lane), col_b = k64_head_row(raw, 2, lane), rho_raw = k64_head_row(raw, 3, lane)
        if constexpr (VARIANT <= 1) {
            k64_two_points(s0, s1, s2, lane, rx_s);
            FragK ps;
            make_pe_sun_k64(rx_s, gq, ps);
            FragK sA[KW2], sB[KW2];
            I8_SOLAR(LAYER, x1f, &ps, sA, sB, raw, rx_s, HEAD_OUT(););
            if constexpr (VARIANT == 1) sv_raw = k64_head_row(raw, 0, lane);
        } else {
            HEAD_OUT();
        }
        if constexpr (VARIANT == 0) {
            I8_ADJUST(LAYER, x1f, hA, hB, raw, sv_raw = k64_head_row(raw, 0, lane););
#pragma unroll
            for (int i = 0; i < 3 * C_MAX; ++i) adj[i] = k64_head_row(raw, i, lane);
        }
#undef HEAD_OUT
#undef LAYER
#undef PEND_T
#undef HAND
#undef TAB
#undef SHAPE
        if constexpr (VARIANT == 3) {
            RAYSUM_PASS_END(rs, A, tile, pass, passes, NW2, wave, wave, NW2, true, lane, rho_raw, x0, x1, x2, tab_lds + A.bias_floats);
        } else {
            if (h == 0 && valid) store_field_outputs<VARIANT>(A.out, n, C, x0, x1, x2, col_r, col_g, col_b, rho_raw, sv_raw, adj, pcls);
            tile += gridDim.x;
        }
    }
    __builtin_amdgcn_s_setprio(0);
}

// the persistent tile loop of one wave group (PHASE: see run_layer8x2); the two groups run two copies of the code
template <int W, int VARIANT, int PHASE>
__device__ __forceinline__ void field_tiles2(const MlpArgs& A, Ring2& rg, lds_char* lds, __attribute__((address_space(3))) float* tab_lds,
                                             int wave, int lane) {
    constexpr int C_MAX = kMaxClasses;
    constexpr int W2 = W / 2;
    const int h = lane >> 5;
    const int C = A.n_classes;
    // VARIANT 3 (ray visibility, mlp_device.h RaySum): a "tile" is a group of NW2 rays, walked in passes of 32 samples
    const int64_t n_tiles = field_tiles(A.n, VARIANT, TILE2, NW2);
    const int passes = VARIANT == 3 ? (A.n_samples + 31) / 32 : 1;
    int pass = 0;
    RaySum rs;
    for (int64_t tile = blockIdx.x; tile < n_tiles;) {
        const int64_t n = tile * TILE2 + wave * 32 + (lane & 31);
        const bool valid = n < A.n;
        const int64_t nc = valid ? n : A.n - 1;
        const int64_t g = VARIANT == 3 ? 0 : nc / A.group_size;

        float x0, x1, x2;
        if constexpr (VARIANT == 3) raysum_point(rs, A, tile, NW2, wave, pass, lane, x0, x1, x2);
        else field_point(A, nc, x0, x1, x2);
        float s0, s1, s2, pcls[C_MAX];
        field_tile_inputs<VARIANT>(A, g, s0, s1, s2, pcls);
        Frag8 pe[PEPOS_KS8];
        make_pe_pos8<VARIANT == 3>(x0, x1, x2, h, pe);

        constexpr int KW = W / 32, KW2 = W2 / 32;
        Frag8 hA[KW], hB[KW];
        f32x16 raw;
        Boundary bd;      // a layer's last block and the next layer's first weight fragments on their way across the boundary (run_layer8x2)
        // The lists of mlp_i8_device.h.  Everything a line does not name comes from the FMT_I8 shape of its layer; the carry a layer receives from that
        // of layer L - 1: HAND(L) = field_carries: layer L hands its last block to its successor in the chain (one flag per boundary, read by both sides).
#define SHAPE(L) field_layer(W, C_MAX, L, FMT_I8)
#define TAB(L) prog_table_start(PROG_FIELD, W, C_MAX, L)
#define HAND(L) (L >= F_FC1 && field_carries(W, VARIANT, C_MAX, L))
#define PEND_T(P) std::conditional_t<HAND(P), Carry<TAB(P), SHAPE(P).nb(), layer_sine(SHAPE(P)), layer_reads_raw(SHAPE(P)), field_feeds_next(P)>, NoCarry>
        // the weight pipeline runs across every boundary of the chain where the pair counts allow it (all of them from W = 128 on)
        constexpr bool XPF = KW2 >= PFX && KW2 % PFX == 0;
#define LAYER(L, IN0, IN1, OUT, RAW, RX, PO, PR, PX)                                                                                                 \
    run_layer8x2<SHAPE(L).nb(), SHAPE(L).ks0, SHAPE(L).ks1, layer_sine(SHAPE(L)), layer_reads_raw(SHAPE(L)), PHASE, VARIANT == 3, PEND_T(L - 1), HAND(L), \
                 XPF && L != F_FC1, XPF && L != field_last(VARIANT)>(rg, A.stream, A.stream_bytes, lds, tab_lds, tab_lds + TAB(L), IN0, IN1, OUT, RAW, bd, \
                                                                     (CarryDst{PO, PR, PX}), wave, lane, RX)
        const float rx_p[3] = {x0, x1, x2}, rx_s[3] = {s0, s1, s2};      // raw coordinates: fp32, no digit range
        Frag8 x1f[KW2];
        I8_TRUNK(LAYER, pe, hA, hB, x1f, &raw, rx_p);
        // the head's regs 0..2 colour, 3 density (lane-half 0).  With the solar branch behind it the head's block finishes inside fc_solar_1 (which
        // does not read it: spread over the whole block), so `raw` is read behind that layer.
        float col_r, col_g, col_b, rho_raw;
        float sv_raw = 0.f;
        float adj[3 * C_MAX];
#pragma unroll
        for (int i = 0; i < 3 * C_MAX; ++i) adj[i] = 0.f;
        if constexpr (VARIANT <= 1) {
            Frag8 ps[PESUN_KS8];
            make_pe_sun8(s0, s1, s2, h, ps);
            Frag8 sA[KW2], sB[KW2];
            // fc_solar_4's one block finishes inside adjust_layer_1 (variant 0), which reads x1f, not the solar branch
            I8_SOLAR(LAYER, x1f, ps, sA, sB, &raw, rx_s, col_r = raw[0], col_g = raw[1], col_b = raw[2], rho_raw = raw[3];);
            if constexpr (VARIANT == 1) sv_raw = raw[0];
        } else {
            col_r = raw[0], col_g = raw[1], col_b = raw[2], rho_raw = raw[3];
        }
        if constexpr (VARIANT == 0) {
            I8_ADJUST(LAYER, x1f, hA, hB, &raw, sv_raw = raw[0];);
#pragma unroll
            for (int i = 0; i < 3 * C_MAX; ++i) adj[i] = raw[i];
        }
#undef LAYER
#undef PEND_T
#undef HAND
#undef TAB
#undef SHAPE
        if constexpr (VARIANT == 3) {
            RAYSUM_PASS_END(rs, A, tile, pass, passes, NW2, wave, wave, NW2, true, lane, rho_raw, x0, x1, x2, tab_lds + A.bias_floats);
        } else {
            if (h == 0 && valid) store_field_outputs<VARIANT>(A.out, n, C, x0, x1, x2, col_r, col_g, col_b, rho_raw, sv_raw, adj, pcls);
            tile += gridDim.x;
        }
    }
    __builtin_amdgcn_s_setprio(0);
}

template <int W, int VARIANT>
static hipError_t launch_mlp_i8x2_t(const MlpArgs& a, int n_cu, hipStream_t st) {
    return launch_fused(mlp_i8x2_kernel<W, VARIANT>, field_tiles(a.n, VARIANT, TILE2, NW2), 64 * NW2,
                        RING2_D * kChunkBytes + a.bias_floats * 4 + kVoteBytes, a, n_cu, st);
}

hipError_t launch_mlp_i8x2(int W, int variant, const MlpArgs& a, int n_cu, hipStream_t st) {
#define CASE(Wv)                                                              \
    if (W == Wv) {                                                            \
        if (variant == 0) return launch_mlp_i8x2_t<Wv, 0>(a, n_cu, st);       \
        if (variant == 1) return launch_mlp_i8x2_t<Wv, 1>(a, n_cu, st);       \
        if (variant == 3) return launch_mlp_i8x2_t<Wv, 3>(a, n_cu, st);       \
        return launch_mlp_i8x2_t<Wv, 2>(a, n_cu, st);                         \
    }
    CASE(64)
    CASE(256)
#undef CASE
    return hipErrorInvalidValue;
}

}  // namespace snerf
