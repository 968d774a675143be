// What the bf16x3 row GEMMs (gemm.hip, gemm16.hip, gemm_areg.hip) share beyond the types of gemm_common.h.
//   device: the block -> work mapping, the weights -> LDS copy, the column-sum reduction, the activation-backward loads and
//           per-element finish, and the one fragment-split kernel;
//   host:   the switches (read once), the routing plan of launch_gemm_bf16x3 (which kernel, which instance, grid, LDS, split
//           layout - every decision made in plan_gemm_rows, gemm.hip), the CU count, the "opt in to large LDS, then launch" helper.
// Device pieces that hipcc compiles to the same instructions as the written-out code are functions.  The others are MACROS:
// as functions they compiled the kernels around them to different code (other register numbers, other s_waitcnt placement, other
// scratch sizes in the activation-backward forms); a macro hands the compiler the text the kernels held before (as mlp_device.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm_common.h"
#include "train.h"

namespace snerf {

// ---------------------------------------------------------------------------------------------------------------------
// Fragment-order split of the weights Bt[n][k] = W[n][k] (transpose = 0, W is [rows x cols]) or W[k][n] (transpose = 1) into bf16
// hi / lo: fragment tk = 1 KiB hi then 1 KiB lo, lane l owns 16 bytes = 8 bf16 (e = 0..7).  The three layouts differ in the order of
// the fragments and in the lane -> (n, k) map:
//   Tile32   (gemm_rows_kernel, gemm_rows_full_kernel; 32x32x16 MFMA): n-tile T (32 columns) major, k-step ks (16 k) minor;
//            lane (r = l & 31, h = l >> 5) owns Bt[32 T + r][16 ks + 8 h + 0..7].
//   KMajor32 (gemm_areg_kernel): the lane layout of Tile32, the fragments k-major - pair (ks, T) at ks * n_tiles + T - so that the
//            weights of one k-step for all n-tiles are one contiguous piece of the stream.
//   Tile16   (gemm_rows16_kernel; 16x16x32 MFMA): n-tile T (16 columns) major, k-step ks (32 k) minor; lane (g = l >> 4, j = l & 15)
//            owns Bt[16 T + j][32 ks + kmap(g, e)], kmap(g, e) = 4 g + e (e < 4), 16 + 4 g + (e - 4) (e >= 4) - so a lane's A values are
//            two 16-byte loads, at byte 16 g and byte 64 + 16 g of the 128-B k-step of its row.  n_tiles / ksteps count 16-column
//            tiles and 32-k steps here.
enum class SplitLayout : int { Tile32, Tile16, KMajor32 };

template <SplitLayout L>
__global__ void split_weights_kernel(const float* W, int rows, int cols, int transpose, uint16_t* frag, int n_tiles, int ksteps) {
    const int64_t total = (int64_t)n_tiles * ksteps * 512;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int e = (int)(i & 7), lane = (int)((i >> 3) & 63);
        const int64_t tk = i >> 9;
        const int ks = (int)(L == SplitLayout::KMajor32 ? tk / n_tiles : tk % ksteps);
        const int T = (int)(L == SplitLayout::KMajor32 ? tk % n_tiles : tk / ksteps);
        int n, k;
        if (L == SplitLayout::Tile16) {
            const int g = lane >> 4;
            n = T * 16 + (lane & 15);
            k = ks * 32 + (e < 4 ? 4 * g + e : 16 + 4 * g + (e - 4));
        } else {
            n = T * 32 + (lane & 31);
            k = ks * 16 + (lane >> 5) * 8 + e;
        }
        float v = 0.f;
        if (!transpose) { if (n < rows && k < cols) v = W[(int64_t)n * cols + k]; }
        else { if (k < rows && n < cols) v = W[(int64_t)k * cols + n]; }
        const __bf16 h = (__bf16)v;
        const __bf16 l = (__bf16)(v - (float)h);
        uint16_t* dst = frag + tk * 1024 + lane * 8 + e;
        dst[0] = __builtin_bit_cast(uint16_t, h);
        dst[512] = __builtin_bit_cast(uint16_t, l);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// block -> (XCD, slot on the XCD) -> (n-group `grp`, `worker`): all n-groups of a worker share an XCD (and its L2), so the second
// reader of a row tile hits that XCD's L2.  Blocks past the last whole worker of their XCD leave the kernel.  (Macro: see the head.)
#define SNERF_ROWS_BLOCK_MAP(n_groups_)                                                               \
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, slots = gridDim.x >> 3;                   \
    const int workers_per_xcd = slots / (n_groups_);                                                  \
    if (slot >= workers_per_xcd * (n_groups_)) return;                                                \
    const int grp = slot % (n_groups_), worker = (slot / (n_groups_)) * 8 + xcd, n_workers = workers_per_xcd * 8

// The NT_ n-tiles of fragments of n-group `grp` (KS k-steps each, 128 16-byte pieces per fragment) -> LDS, straight copy by NTH_
// threads: eight loads per thread in flight at a time instead of one round trip per NTH_ * 16 bytes.  Uses g, lds_w, grp, KS, tid.
// (Macro: as a function taking the two pointers it changed the address arithmetic of the copy loop in every kernel.)
#define SNERF_ROWS_WEIGHTS_TO_LDS(NT_, NTH_)                                                          \
    {                                                                                                 \
        const u32x4* src = (const u32x4*)(g.frag + (int64_t)grp * NT_ * KS * 1024);                   \
        u32x4* dst = (u32x4*)lds_w;                                                                   \
        const int n16 = NT_ * KS * 128;                                                               \
        int i0 = tid;                                                                                 \
        for (; i0 + 7 * (NTH_) < n16; i0 += (NTH_) * 8) {                                             \
            u32x4 v[8];                                                                               \
            _Pragma("unroll") for (int q = 0; q < 8; ++q) v[q] = src[i0 + q * (NTH_)];                \
            _Pragma("unroll") for (int q = 0; q < 8; ++q) dst[i0 + q * (NTH_)] = v[q];                \
        }                                                                                             \
        for (; i0 < n16; i0 += (NTH_)) dst[i0] = src[i0];                                             \
    }

// Per-column sums of a workgroup -> double atomics on g.stats [2][N] (forward: sum(v - shift), sum((v - shift)^2); ACT: sum v,
// sum v*xhat).  The weights are no longer needed: their LDS holds the cross-wave reduction red[waves][NT][2][W].  W = 32 or 16
// columns per n-tile: the 64 / W lanes that share a column are folded by shuffles, the lanes `first_` (row group 0) publish column
// `col_`; A_ / B_ are the two sums of n-tile j as this lane holds them, OK_ whether n-tile j of this group exists.
// Uses g, lds_w, tid, wave, grp of the kernel.  (Macro: see the head.)
#define SNERF_ROWS_COLUMN_SUMS(W_, NT_, WAVES_, A_, B_, first_, col_, OK_)                                          \
    if (g.stats) {                                                                                                  \
        __syncthreads();                                                                                            \
        float* red = (float*)lds_w;                                                                                 \
        _Pragma("unroll") for (int j = 0; j < NT_; ++j) {                                                           \
            float a = A_, b = B_;                                                                                   \
            if (W_ == 16) { a += __shfl_xor(a, 16, 64); b += __shfl_xor(b, 16, 64); }                               \
            a += __shfl_xor(a, 32, 64); b += __shfl_xor(b, 32, 64);                                                 \
            if (first_) {                                                                                           \
                red[((wave * NT_ + j) * 2 + 0) * W_ + col_] = a;                                                    \
                red[((wave * NT_ + j) * 2 + 1) * W_ + col_] = b;                                                    \
            }                                                                                                       \
        }                                                                                                           \
        __syncthreads();                                                                                            \
        if (tid < NT_ * 2 * W_) {                                                                                   \
            constexpr int LW = W_ == 32 ? 5 : 4;                                                                    \
            const int j = tid >> (LW + 1), which = (tid >> LW) & 1, c = tid & (W_ - 1);                             \
            double s = 0.0;                                                                                         \
            _Pragma("unroll") for (int w = 0; w < WAVES_; ++w) s += (double)red[((w * NT_ + j) * 2 + which) * W_ + c]; \
            const int64_t n = (int64_t)(grp * NT_ + j) * W_ + c;                                                    \
            if ((OK_) && n < g.N) atomicAdd(g.stats + which * g.N + n, s);                                          \
        }                                                                                                           \
    }

// Activation backward in the epilogue of a full-tile kernel (ACT): the value produced is dL/dH of the SineLayer below; times
// cos(2 pi (a z + b)) of that layer's pre-activation z it is dL/d(arg), and the column sums are sum v and sum v * xhat,
// xhat = (z - mu) istd.  c = [a, b, mu, istd] of the column (mu = istd = 0 for a layer without BatchNorm).
// The NE_ pre-activations of this lane's column at n-tile byte offset joff_ (column n_): element e sits RO_ rows (an expression in e)
// below the wave's first row `rowu` - through the buffer descriptor rs_z + lane offset lz when no row of the workgroup tile is masked
// (INTERIOR), from clamped addresses otherwise (ROWM_: the row, an expression in ro).  (Macro: see the head.)
#define SNERF_ROWS_ACT_FETCH_Z(z_, NE_, RO_, ROWM_, joff_, n_)                                                      \
    _Pragma("unroll") for (int e = 0; e < NE_; ++e) {                                                               \
        const int64_t ro = RO_;                                                                                     \
        if (INTERIOR) {                                                                                             \
            z_[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_z, lz + (joff_), (int)((rowu + ro) * g.eld * 4), 0)); \
        } else {                                                                                                    \
            int64_t m = ROWM_;                                                                                      \
            m = m < g.M ? m : g.M - 1;                                                                              \
            z_[e] = g.ez[m * g.eld + (n_)];                                                                         \
        }                                                                                                           \
    }
__device__ __forceinline__ float rows_act_bwd(float v, float z, const float (&c)[4]) {
    return v * __builtin_amdgcn_cosf(__builtin_fmaf(c[0], z, c[1]));
}
__device__ __forceinline__ void rows_act_bwd_sums(float v, float z, const float (&c)[4], bool ok, float& st1, float& st2) {
    const float s1 = v, s2 = v * ((z - c[2]) * c[3]);
    st1 += ok ? s1 : 0.f;
    st2 += ok ? s2 : 0.f;
}

// ---------------------------------------------------------------------------------------------------------------------
// Host side.

// Environment switches of the row GEMMs, read once per process (INTEGRATION.md lists them).
struct RowsSwitches {
    int areg;           // SNERF_GEMM_AREG (1): the AGPR-accumulator kernel on N = 512 or K > 256; 0 off; 2 every shape it takes
    int areg_act;       // SNERF_GEMM_AREG_ACT (1): also its activation-backward form; 0 keeps the column-group kernel for those
    int areg_hv;        // SNERF_AREG_HV (2): two waves per SIMD for the forward forms at N = 512; 1 the one-wave form there too
    int full;           // SNERF_GEMM_FULL (1): the pipelined full-tile kernels wherever the shape allows; 0 the general kernel
    int pf;             // SNERF_GEMM_PF (0 = by shape): 2 | 4 | 8 k-steps of A in flight in gemm_rows_full_kernel
    int gemm16;         // SNERF_GEMM16 (1): the 16x16x32 form on the wide layers; 0 the 32x32x16 full-tile kernel
    int gemm16_k320;    // SNERF_GEMM16_K320 (1): the K = 320 layer's forward on the 16x16x32 form too
    int snake;          // SNERF_SNAKE (1): streaming launches alternate their direction (stream_direction); 0 always forwards
};
const RowsSwitches& rows_switches();

enum class RowsKernel : int { AREG, ROWS16, FULL, GENERAL };      // gemm_areg_kernel, gemm_rows16_kernel, gemm_rows_full_kernel, gemm_rows_kernel
// What launch_gemm_bf16x3 does for one GemmX: written by plan_gemm_rows (which launches nothing), executed by run_gemm_rows.
struct RowsPlan {
    RowsKernel kernel;
    int nt, pf, aol, act;      // the kernel's template arguments NT, PF (PFA; 0: GENERAL has none), AOL, ACT
    int hv;                    // AREG: waves per SIMD (template argument HV)
    unsigned grid;
    size_t lds;                // dynamic LDS bytes
    int tab_lds;               // GemmX::tab_lds for the kernel
    SplitLayout split;         // fragment order of raw weights (GemmX::W) for this kernel
    bool zero_bn;              // ACT without BatchNorm statistics: emu / eistd point at zeros
};
hipError_t plan_gemm_rows(const GemmX& g, const RowsSwitches& sw, RowsPlan& p);

// compile-time geometry of the other translation units (diagnostic builds change it per source: SNERF_R16_RT, SNERF_AR_D)
int gemm_rows16_waves();                                              // gemm16.hip: waves per workgroup (8; 16 with SNERF_R16_RT=1)
void gemm_areg_geometry(int* tile_rows, size_t* ring_bytes);          // gemm_areg.hip: rows per workgroup tile, bytes of the weight ring
// the kernels of the other translation units: the instance p names, on p.grid workgroups with p.lds bytes
hipError_t launch_gemm_rows16(const GemmX& gx, const RowsPlan& p, hipStream_t st);
hipError_t launch_gemm_areg(const GemmX& gx, const RowsPlan& p, hipStream_t st);      // gx.frag holds the KMajor32 stream

// CUs of the current device, read once (256 if the query fails).  whole_xcds: rounded down to a multiple of 8, at least 8 - the
// kernels that map blocks to (XCD, slot) and the weight gradient want the same number of workgroups on every XCD.
int gemm_device_cus(bool whole_xcds);

// fragment split of raw weights, at most max_blocks workgroups (grid-stride)
hipError_t launch_split_weights(SplitLayout layout, const float* W, int rows, int cols, bool transpose, uint16_t* frag, int n_tiles, int ksteps,
                                int max_blocks, hipStream_t st);

// Opt in to more than 64 KiB of dynamic LDS (once per kernel), then launch.
template <auto Kernel, int MaxLds = 160 * 1024, typename Arg>
inline hipError_t launch_big_lds(dim3 grid, dim3 block, size_t lds, hipStream_t st, const Arg& arg) {
    static bool opted_in = false;
    if (!opted_in) {
        hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, MaxLds);
        if (e != hipSuccess) return e;
        opted_in = true;
    }
    hipLaunchKernelGGL(Kernel, grid, block, lds, st, arg);
    return hipGetLastError();
}

}  // namespace snerf
