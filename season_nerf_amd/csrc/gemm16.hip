// Full-tile row GEMM on v_mfma_f32_16x16x32_bf16 (its own translation unit: see the comment at the kernel).  Launched by run_gemm_rows (gemm.hip) with the
// instance plan_gemm_rows chose; the pieces it shares with the 32x32x16 kernels are in gemm_rows.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "gemm_rows.h"
#include "train.h"

#ifndef SNERF_STORE_AUX
#define SNERF_STORE_AUX 0  // cache policy of the epilogue stores (buffer instruction aux bits: 1 sc0, 2 nt, 16 sc1)
#endif
#ifndef SNERF_ABL16
#define SNERF_ABL16 0      // timing-only ablations of scratch builds (tools/variants.py): 1 no MFMAs, 2 no stores, 4 no A refills, 8 no sin / split, 16 no LDS weight reads
#endif

namespace snerf {

// ---------------------------------------------------------------------------------------------------------------------
// The same full-tile row GEMM on v_mfma_f32_16x16x32_bf16.  Why a second MFMA shape: the vector-memory path, not HBM or the
// matrix pipe, bounds the 32x32x16 form.  Its A operand puts one ROW on every lane of a half-wave - a 1 KiB load
// instruction touches 64 different 128-B lines (147 cycles per instruction and CU, tools/probes/ta_rate.hip) - and every A
// byte is loaded by two column groups.  The 16x16x32 A operand has 16 rows x 4 lanes: with the k order chosen below the four
// lanes of a row read 64 contiguous bytes per instruction (quad-coalesced: 67 cycles), from the SAME row-major activations.
// The accumulator of a 16x16 tile (lane (g, j): column j, rows 4g .. 4g+3) stores as four 64-B row segments per instruction,
// at the per-byte rate of the 32x32 form's two 128-B segments (17 against 16 cycles per 256 B).  Arithmetic, summation order
// inside a product (hi*hi last) and results differ from the 32x32x16 kernel only by the order of the k terms inside a 32-k step.
//   fragment order: SplitLayout::Tile16 of split_weights_kernel (gemm_rows.h) - a lane's A values are two 16-byte loads, at byte 16 g and byte
//   64 + 16 g of the 128-B k-step of its row.
// A wave owns 32 rows = two 16-row tiles (each weight fragment read from LDS serves both); 8 waves = 256 rows per workgroup tile.
__device__ __forceinline__ void a16_issue(const float* p, f32x4& x, f32x4& y) {       // k = 4g .. 4g+3 and 16+4g .. 16+4g+3 of a 32-k step
    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:64" : "=&v"(x), "=&v"(y) : "v"(p));
}
template <int N>
__device__ __forceinline__ void a16_wait(f32x4& x0, f32x4& y0, f32x4& x1, f32x4& y1) {
    asm volatile("s_waitcnt vmcnt(%4) ; a16_wait %0 %1 %2 %3" : "+v"(x0), "+v"(y0), "+v"(x1), "+v"(y1) : "n"(N));
}
template <int N>
__device__ __forceinline__ void a16_wait(f32x4& x0, f32x4& y0) {
    asm volatile("s_waitcnt vmcnt(%2) ; a16_wait %0 %1" : "+v"(x0), "+v"(y0) : "n"(N));
}
#ifndef SNERF_R16_RT
#define SNERF_R16_RT 2      // 16-row tiles per wave: 2 = 8 waves x 32 rows (two waves per SIMD), 1 = 16 waves x 16 rows (four per SIMD)
#endif
constexpr int R16_RT = SNERF_R16_RT, R16_WAVES = RO_ROWS / (16 * R16_RT);
template <int N>
__device__ __forceinline__ void a16_wait_slot(f32x4 (&x)[R16_RT], f32x4 (&y)[R16_RT]) {
    if constexpr (R16_RT == 2) a16_wait<N>(x[0], y[0], x[1], y[1]);
    else a16_wait<N>(x[0], y[0]);
}

// NT: 16-column n-tiles per group (8 = 128 columns).  PF: 32-k steps of A in flight.  AOL / ACT as in gemm_rows_full_kernel.
template <int NT, int PF, int AOL, int ACT>
__global__ __launch_bounds__(64 * R16_WAVES) void gemm_rows16_kernel(const GemmX g) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_w[];
#ifdef SNERF_STAMP16
    const uint64_t stamp_entry = __builtin_amdgcn_s_memrealtime();
#endif
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int jj = lane & 15, gq = lane >> 4;
    const int KS = g.ksteps >> 1;                                   // 32-k steps (multiple of PF)
    const int n_groups = (2 * g.n_tiles) / NT;
    SNERF_ROWS_BLOCK_MAP(n_groups);

    SNERF_ROWS_WEIGHTS_TO_LDS(NT, 64 * R16_WAVES)
    const uint8_t* lds_tab = lds_w + (size_t)NT * KS * 2048;
    if (AOL == 1) {
        float* dst = (float*)lds_tab;
        for (int i = tid; i < 2 * g.act_cols; i += 64 * R16_WAVES) dst[i] = g.act_tab[i];
    }
    // per-column constants of this group's NT * 16 columns, behind the table: the epilogue reads them from LDS - a global load there
    // would make hipcc wait for vmcnt(0), i.e. for the previous tile's stores and every prefetched operand of the next one
    float* lds_col = (float*)(lds_tab + (AOL ? (size_t)g.act_cols * 8 : 0));      // [bias | etab a | etab b | mu | istd][NT * 16]
    for (int i = tid; i < NT * 16; i += 64 * R16_WAVES) {
        const int64_t n = (int64_t)grp * NT * 16 + i;
        const bool in = n < g.N;
        lds_col[i] = (!ACT && g.bias && in) ? g.bias[n] : 0.f;
        if (ACT) {
            lds_col[NT * 16 + i] = in ? g.etab[n] : 0.f;
            lds_col[2 * NT * 16 + i] = in ? g.etab[g.N + n] : 0.f;
            lds_col[3 * NT * 16 + i] = in ? g.emu[n] : 0.f;
            lds_col[4 * NT * 16 + i] = in ? g.eistd[n] : 0.f;
        }
    }
    const int col0 = grp * NT * 16 + jj;                            // this lane's column of n-tile 0
    __syncthreads();

    const int64_t n_row_tiles = (g.M + RO_ROWS - 1) / RO_ROWS;
    float st1[NT], st2[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) st1[j] = st2[j] = 0.f;
#ifdef SNERF_STAMP16      // diagnostic build: shader clock held inside the tile loop = d(s_memtime) / d(s_memrealtime) x 100 MHz
    const uint64_t stamp_c0 = __builtin_amdgcn_s_memtime(), stamp_r0 = __builtin_amdgcn_s_memrealtime();
#endif

    auto a_ptr = [&](int64_t rt, int half) {
        int64_t m = (g.reverse ? n_row_tiles - 1 - rt : rt) * RO_ROWS + wave * (16 * R16_RT) + half * 16 + jj;
        m = m < g.M ? m : g.M - 1;                                  // loads stay in bounds, stores are masked
        return g.A + m * g.lda + gq * 4;
    };
    // epilogue addressing through buffer instructions (see gemm_rows_full_kernel): lane offset + scalar row offset + immediate
    const bool nok0 = NT > 1 || col0 < g.N;                       // thin head (N < 16): out-of-range lanes store nowhere
    const int lc = nok0 ? (int)(4 * gq * g.ldc + col0) * 4 : (int)0x80000000;
    const int lz = ACT ? (int)(4 * gq * g.eld + col0) * 4 : 0;
    const __amdgpu_buffer_rsrc_t rs_c = __builtin_amdgcn_make_buffer_rsrc((void*)g.C, 0, (int)(g.M * g.ldc * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_z = __builtin_amdgcn_make_buffer_rsrc((void*)(ACT ? g.ez : g.A), 0, -1, 0x00020000);
    int64_t rt = worker;
    const float* arow[R16_RT];
#pragma unroll
    for (int h = 0; h < R16_RT; ++h) arow[h] = a_ptr(rt < n_row_tiles ? rt : n_row_tiles - 1, h);
    f32x4 px[PF][R16_RT], py[PF][R16_RT];
#pragma unroll
    for (int d = 0; d < PF; ++d)
#pragma unroll
        for (int h = 0; h < R16_RT; ++h) a16_issue(arow[h] + d * 32, px[d][h], py[d][h]);

#ifdef SNERF_PHASE16       // diagnostic build: where one wave's time goes (shader cycles: load wait | convert + refill | LDS + MFMA issue | epilogue)
#define SNERF_PH(x) __builtin_amdgcn_sched_barrier(0); const uint64_t x = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0)
    uint64_t ph_wait = 0, ph_conv = 0, ph_mfma = 0, ph_epi = 0, ph_steps = 0;
    const uint64_t ph_t0 = __builtin_amdgcn_s_memtime();
#else
#define SNERF_PH(x)
#endif
    for (; rt < n_row_tiles; rt += n_workers) {
        const int64_t rn = rt + n_workers;
        const float* anext[R16_RT];
#pragma unroll
        for (int h = 0; h < R16_RT; ++h) anext[h] = a_ptr(rn < n_row_tiles ? rn : rt, h);
        f32x4 acc[R16_RT][NT];
#pragma unroll
        for (int h = 0; h < R16_RT; ++h)
#pragma unroll
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[h][j][e] = 0.f;
        for (int ks0 = 0; ks0 < KS; ks0 += PF) {
            const bool last = ks0 + PF >= KS;
            const float* srcs[R16_RT];
#pragma unroll
            for (int h = 0; h < R16_RT; ++h) srcs[h] = last ? anext[h] : arow[h] + (ks0 + PF) * 32;
#pragma unroll
            for (int d = 0; d < PF; ++d) {
                const int ks = ks0 + d;
                f32x4 ta[2], tb[2];                                  // AOL: [a | b] of this lane's 8 k values (shared by both row tiles)
                if (AOL) {
                    int k0 = ks * 32 + gq * 4;
                    k0 = k0 + 20 <= g.act_cols ? k0 : 0;           // clamped: the loads are unconditional (act_cols is a multiple of 32 here)
                    const float* tp = (const float*)lds_tab + k0;
                    ta[0] = *(const f32x4*)tp; ta[1] = *(const f32x4*)(tp + 16);
                    tb[0] = *(const f32x4*)(tp + g.act_cols); tb[1] = *(const f32x4*)(tp + g.act_cols + 16);
                }
                SNERF_PH(q0);
#if !(SNERF_ABL16 & 4)
                a16_wait_slot<2 * R16_RT * (PF - 1)>(px[d], py[d]);                  // the PF-1 younger k-steps stay in flight
#endif
                SNERF_PH(q1);
                u32x4 ahi[R16_RT], alo[R16_RT];
#pragma unroll
                for (int h = 0; h < R16_RT; ++h) {
                    float a8[8] = {px[d][h][0], px[d][h][1], px[d][h][2], px[d][h][3], py[d][h][0], py[d][h][1], py[d][h][2], py[d][h][3]};
#if SNERF_ABL16 & 8
                    for (int q = 0; q < 4; ++q) { ahi[h][q] = __builtin_bit_cast(uint32_t, a8[2 * q]); alo[h][q] = __builtin_bit_cast(uint32_t, a8[2 * q + 1]); }
                    continue;
#endif
                    if (AOL) {
                        if (ks * 32 < g.act_cols) {                 // uniform
#pragma unroll
                            for (int e = 0; e < 8; ++e)
                                a8[e] = __builtin_amdgcn_sinf(__builtin_fmaf(ta[e >> 2][e & 3], a8[e], tb[e >> 2][e & 3]));
                        }
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        uint32_t hh, ll;
                        split2_bf16(a8[2 * q], a8[2 * q + 1], hh, ll);
                        ahi[h][q] = hh;
                        alo[h][q] = ll;
                    }
                }
#if !(SNERF_ABL16 & 4)
#pragma unroll
                for (int h = 0; h < R16_RT; ++h) a16_issue(srcs[h] + d * 32, px[d][h], py[d][h]);      // refill the slot just consumed (next tile's on the last round)
#endif
                __builtin_amdgcn_sched_barrier(0);
                SNERF_PH(q2);
                bf16x8 Ahi[R16_RT], Alo[R16_RT];
#pragma unroll
                for (int h = 0; h < R16_RT; ++h) { Ahi[h] = __builtin_bit_cast(bf16x8, ahi[h]); Alo[h] = __builtin_bit_cast(bf16x8, alo[h]); }
                const uint32_t base = (uint32_t)ks * 2048u + (uint32_t)lane * 16u;
                constexpr int JB = NT < 4 ? NT : 4;                  // weight fragments of four n-tiles in registers at a time
#pragma unroll
                for (int j0 = 0; j0 < NT; j0 += JB) {
                    bf16x8 Bhi[JB], Blo[JB];
#pragma unroll
                    for (int j = 0; j < JB; ++j) {
#if SNERF_ABL16 & 16
                        Bhi[j] = Ahi[0]; Blo[j] = Alo[R16_RT - 1];
#else
                        Bhi[j] = __builtin_bit_cast(bf16x8, *(const u32x4*)(lds_w + base + (uint32_t)(j0 + j) * KS * 2048u));
                        Blo[j] = __builtin_bit_cast(bf16x8, *(const u32x4*)(lds_w + base + (uint32_t)(j0 + j) * KS * 2048u + 1024u));
#endif
                    }
#if SNERF_ABL16 & 1
#pragma unroll
                    for (int j = 0; j < JB; ++j) {      // keep every operand alive with one cheap VALU op per accumulator register group
#pragma unroll
                        for (int h = 0; h < R16_RT; ++h)
                            acc[h][j0 + j][0] += __builtin_bit_cast(float, (h ? __builtin_bit_cast(u32x4, Blo[j])[0] : __builtin_bit_cast(u32x4, Bhi[j])[0]) ^ ahi[h][0] ^ alo[h][1]);
                    }
                    continue;
#endif
#pragma unroll
                    for (int j = 0; j < JB; ++j) {
                        acc[0][j0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Alo[0], Bhi[j], acc[0][j0 + j], 0, 0, 0);
                        if constexpr (R16_RT == 2) acc[R16_RT - 1][j0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Alo[R16_RT - 1], Bhi[j], acc[R16_RT - 1][j0 + j], 0, 0, 0);
                    }
#pragma unroll
                    for (int j = 0; j < JB; ++j) {
                        acc[0][j0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ahi[0], Blo[j], acc[0][j0 + j], 0, 0, 0);
                        if constexpr (R16_RT == 2) acc[R16_RT - 1][j0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ahi[R16_RT - 1], Blo[j], acc[R16_RT - 1][j0 + j], 0, 0, 0);
                    }
#pragma unroll
                    for (int j = 0; j < JB; ++j) {
                        acc[0][j0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ahi[0], Bhi[j], acc[0][j0 + j], 0, 0, 0);
                        if constexpr (R16_RT == 2) acc[R16_RT - 1][j0 + j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(Ahi[R16_RT - 1], Bhi[j], acc[R16_RT - 1][j0 + j], 0, 0, 0);
                    }
                }
#ifdef SNERF_PHASE16
                SNERF_PH(q3);
                ph_wait += q1 - q0; ph_conv += q2 - q1; ph_mfma += q3 - q2; ++ph_steps;
#endif
            }
        }
        // epilogue: D[row = 16 h + 4 gq + e, col = 16 j + jj]
        const int64_t rt_m = g.reverse ? n_row_tiles - 1 - rt : rt;
        const int64_t rowu = rt_m * RO_ROWS + wave * (16 * R16_RT);
        auto epilogue = [&](auto interior_tag) {
            constexpr bool INTERIOR = decltype(interior_tag)::value;      // no row of the workgroup tile is masked: branch-free
            float zt[2][4 * R16_RT], ec[2][4];
            auto fetch = [&](int j, float (&z_)[4 * R16_RT], float (&c_)[4]) {     // ACT: pre-activations and [a, b, mu, istd] of column j
                const int64_t n = col0 + 16 * j;
                SNERF_ROWS_ACT_FETCH_Z(z_, 4 * R16_RT, 16 * (e >> 2) + (e & 3), rowu + ro + 4 * gq, j * 64, n)      // element 4 h + e: row 16 h + e
                c_[0] = lds_col[NT * 16 + 16 * j + jj]; c_[1] = lds_col[2 * NT * 16 + 16 * j + jj];
                c_[2] = lds_col[3 * NT * 16 + 16 * j + jj]; c_[3] = lds_col[4 * NT * 16 + 16 * j + jj];      // (zeros for a layer without BatchNorm)
            };
            if (ACT) fetch(0, zt[0], ec[0]);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int64_t n = col0 + 16 * j;
                // bias of this lane's column: fetched here (L1-resident), not held in registers across the k-loop
                // plain form: v = alpha acc + (alpha bias) in one fma, and the BatchNorm sums of v - alpha bias = alpha acc are taken from the
                // accumulator itself (sum acc, sum acc^2; scaled by alpha, alpha^2 once, after the tile loop): 3 vector instructions per element
                const float abj = ACT ? 0.f : g.alpha * lds_col[16 * j + jj];
                if (ACT) {
                    if (j + 1 < NT) fetch(j + 1, zt[(j + 1) & 1], ec[(j + 1) & 1]);
                    __builtin_amdgcn_sched_barrier(0);
                }
#pragma unroll
                for (int h = 0; h < R16_RT; ++h)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int64_t ro = 16 * h + e;
                        float v = ACT ? g.alpha * acc[h][j][e] : __builtin_fmaf(g.alpha, acc[h][j][e], abj);
                        const float z = ACT ? zt[j & 1][4 * h + e] : 0.f;
                        if (ACT) v = rows_act_bwd(v, z, ec[j & 1]);
                        const bool ok = INTERIOR || rowu + ro + 4 * gq < g.M;
                        if (SNERF_ABL16 & 2) {
                            if (v == 123.456f) g.C[0] = v;
                        } else if (INTERIOR) {
                            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), rs_c, lc + j * 64, (int)((rowu + ro) * g.ldc * 4), SNERF_STORE_AUX);
                        } else if (ok && nok0) {
                            g.C[(rowu + ro + 4 * gq) * g.ldc + n] = v;
                        }
                        if (ACT) {
                            rows_act_bwd_sums(v, z, ec[j & 1], ok, st1[j], st2[j]);
                        } else {
                            const float dd = acc[h][j][e];
                            st1[j] += ok ? dd : 0.f;
                            st2[j] += ok ? dd * dd : 0.f;
                        }
                    }
                if (ACT) __builtin_amdgcn_sched_barrier(0);
            }
        };
        if (ACT) {      // this variant's epilogue may spill registers: the prefetched operands must have landed before it may touch them
#pragma unroll
            for (int d = 0; d < PF; ++d) a16_wait_slot<0>(px[d], py[d]);
        }
        SNERF_PH(q4);
        if (rt_m * RO_ROWS + RO_ROWS <= g.M) epilogue(std::true_type{});
        else epilogue(std::false_type{});
#ifdef SNERF_PHASE16
        SNERF_PH(q5);
        ph_epi += q5 - q4;
#endif
#pragma unroll
        for (int h = 0; h < R16_RT; ++h) arow[h] = anext[h];
    }
    // the never-consumed refills of the last round must land before their registers are reused (see gemm_rows_full_kernel)
#pragma unroll
    for (int d = 0; d < PF; ++d) a16_wait_slot<0>(px[d], py[d]);
#ifdef SNERF_PHASE16
    if (g.stats && lane == 0 && (wave == 0 || wave == R16_WAVES / 2) && blockIdx.x < 256) {
        double* o = g.stats + 2 * g.N + 1024 + (blockIdx.x * 2 + (wave != 0)) * 6;
        o[0] = (double)ph_wait; o[1] = (double)ph_conv; o[2] = (double)ph_mfma; o[3] = (double)ph_epi;
        o[4] = (double)(__builtin_amdgcn_s_memtime() - ph_t0); o[5] = (double)ph_steps;
    }
#endif
#ifdef SNERF_STAMP16
    if (g.stats && tid == 0 && blockIdx.x < 256) {     // per workgroup, behind the column sums: cycles of the tile loop, its start and end in 100 MHz ticks
        g.stats[2 * g.N + 3 * blockIdx.x] = (double)stamp_entry;
        g.stats[2 * g.N + 3 * blockIdx.x + 1] = (double)stamp_r0;
        g.stats[2 * g.N + 3 * blockIdx.x + 2] = (double)__builtin_amdgcn_s_memrealtime();
    }
#endif
    // (the plain form summed the accumulators: scaled by alpha, alpha^2 here, once)
    SNERF_ROWS_COLUMN_SUMS(16, NT, R16_WAVES, ACT ? st1[j] : g.alpha * st1[j], ACT ? st2[j] : (g.alpha * g.alpha) * st2[j], gq == 0, jj, true)
#ifdef SNERF_STAMP16
    __syncthreads();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every store and atomic of this wave acknowledged
    if (g.stats && tid == 0 && blockIdx.x < 256) g.stats[2 * g.N + 768 + blockIdx.x] = (double)__builtin_amdgcn_s_memrealtime();
#endif
}

template <int NT, int PF>
static hipError_t launch_rows16(const GemmX& gx, const RowsPlan& p, hipStream_t st) {
    const dim3 grid(p.grid), block(64 * R16_WAVES);
    if constexpr (PF == 4) {          // only the activation-on-load form fits four k-steps of prefetch without scratch
        if (p.act || !p.aol) return hipErrorInvalidValue;
        return launch_big_lds<gemm_rows16_kernel<NT, PF, 1, 0>>(grid, block, p.lds, st, gx);
    } else {
        if (p.act) return launch_big_lds<gemm_rows16_kernel<NT, PF, 0, 1>>(grid, block, p.lds, st, gx);
        if (p.aol) return launch_big_lds<gemm_rows16_kernel<NT, PF, 1, 0>>(grid, block, p.lds, st, gx);
        return launch_big_lds<gemm_rows16_kernel<NT, PF, 0, 0>>(grid, block, p.lds, st, gx);
    }
}
template <int NT>
static hipError_t launch_rows16_nt(const GemmX& gx, const RowsPlan& p, hipStream_t st) {
    return p.pf == 4 ? launch_rows16<NT, 4>(gx, p, st) : p.pf == 2 ? launch_rows16<NT, 2>(gx, p, st) : p.pf == 1 ? launch_rows16<NT, 1>(gx, p, st) : hipErrorInvalidValue;
}

int gemm_rows16_waves() { return R16_WAVES; }

// gx: as run_gemm_rows prepared it (weights split in the Tile16 order, K in whole 32-k steps, N = 32 n_tiles).  p.nt: 16-column n-tiles per column
// group - 8 (128 columns; K <= 256) or 4 (64 columns: the K = 320 layer, forwards only)
hipError_t launch_gemm_rows16(const GemmX& gx, const RowsPlan& p, hipStream_t st) {
    if (p.nt == 4 && p.act) return hipErrorInvalidValue;
    return p.nt == 4 ? launch_rows16_nt<4>(gx, p, st) : p.nt == 8 ? launch_rows16_nt<8>(gx, p, st) : hipErrorInvalidValue;
}

}  // namespace snerf
