// The three products of a Linear / SineLayer in training - forward, input gradient (dgrad), weight gradient (wgrad) - as ONE description (Product), one routing
// function per product and one builder per kernel argument block.  Host code only: the training engine (from LayerP / Act / ActBelow) and the public
// snerf_linear_* entry points (from their raw arguments) both go through here (train.cpp); where the two deliberately differ, the difference is a field of Policy.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "rows_debug.h"
#include "train.h"

namespace snerf {
// The A/B switches of the training side, read once per process; SNERF_TRAIN_GEMM / SNERF_TRAIN_AOL are per-trainer values, read at create time.
// memops: runtime memory operations instead of the copy / fill kernels (reproduction only, see train.cpp); fused_heads: heads' forward as a stream, colour +
// density heads as one K = 4 product; thin_wgrad / thin_dgrad: a single thin head's weight / input gradient as a stream; dy_bf16: EXPERIMENT (sine_bwd).
struct Switches { bool memops, fused_heads, thin_wgrad, thin_dgrad, dy_bf16; };
inline const Switches& switches() {
    static const Switches s = [] {
        auto on = [](const char* e) { return !(e && e[0] == '0'); };      // default on, off with =0
        const char* m = getenv("SNERF_TRAIN_MEMOPS");
        return Switches{m && m[0] == '1', on(getenv("SNERF_FUSED_HEADS")), on(getenv("SNERF_THIN_WGRAD")), on(getenv("SNERF_THIN_DGRAD")), getenv("SNERF_TRAIN_DY_BF16") != nullptr};
    }();
    return s;
}

struct Policy {          // who calls: every intended difference between the engine and the public entry points
    bool bf16x3;         // error-compensated bf16x3 kernels wanted (engine: the trainer's SNERF_TRAIN_GEMM; public: precision == 1), else exact fp32 everywhere
    int64_t rows_min;    // fewest rows they are used for: the engine sends small (per-ray) batches to exact fp32 (1024), a public call asked for bf16x3 by name (1)
    bool thin_fwd;       // forward may stream: the engine's plain heads and the public call, never a SineLayer of the engine (alpha = 30, statistics)
    bool thin_dgrad;     // input gradient may stream: engine only
};
// activation backward of the SineLayer below, applied by the dgrad that produces that layer's output gradient (z == nullptr: none): its pre-activation z [M, ld],
// its [a | b] table, its BatchNorm mean / istd (nullptr without BatchNorm); sums [2][n_cols] += column sums of the result and of result * xhat
struct Epilogue { const float *z = nullptr, *tab = nullptr, *mu = nullptr, *istd = nullptr; int64_t ld = 0; double* sums = nullptr; };
struct Product {
    int64_t M = 0; int n_in = 0, n_out = 0; float alpha = 1.f;
    const float *W = nullptr, *bias = nullptr; float* dW = nullptr;                    // [n_out, n_in] (ld n_in), [n_out];  wgrad: dW += (ld n_in, or lddw)
    int64_t lddw = 0;                                                                  // wgrad, Rows route: row stride of dW where it is not n_in (0; test hook only)
    // second head: row 3 of W / bias / dW lives here instead (colour rows 0..2 + density row 3 as one K = 4 product; thin route only)
    const float *W3 = nullptr, *bias3 = nullptr; float* dW3 = nullptr;
    // the layer's input [M, ldx];  activation on load: its first tab_cols columns are pre-activations, tab = [a | b];  x_padded: columns n_in .. next multiple of 16 exist and hold zeros
    const float *X = nullptr, *tab = nullptr; int64_t ldx = 0; int tab_cols = 0; bool x_padded = false;
    float* Y = nullptr; int64_t ldy = 0;                                               // forward: the output [M, ldy];  backward: dL/d(output) (written only by the BatchNorm wgrad)
    double* stats = nullptr; float* colsum = nullptr;                                  // forward: BatchNorm sums from the row GEMM's epilogue / column sums from the fp32 GEMM
    float* dX = nullptr; int64_t lddx = 0; int n_cols = 0; bool accumulate = false;    // dgrad: dL/d(input)[:, :n_cols] (ld lddx), added to with `accumulate`
    Epilogue below;                                                                    // dgrad
    const WgradBN* bn = nullptr;                                                       // wgrad: BatchNorm dZ pass folded in (engine only)
    const uint16_t* frag = nullptr;                                                    // scratch for the split weights of the row GEMM
};

// ---- one builder per argument block
inline ThinFwdArgs thin_fwd_args(const Product& p) {
    ThinFwdArgs f{};
    f.In = p.X; f.ldi = p.ldx; f.M = p.M; f.K = p.n_out; f.N = p.n_in; f.alpha = p.alpha; f.Out = p.Y; f.ldo = p.ldy;
    f.W = p.W; f.ldw = p.n_in; f.W3 = p.W3; f.bias = p.bias; f.bias3 = p.bias3; f.tab = p.tab; f.tab_cols = p.tab_cols; f.tab_stride = p.tab_cols;
    return f;
}
inline ThinWgradArgs thin_wgrad_args(const Product& p) {
    ThinWgradArgs a{};
    a.D = p.Y; a.ldd = p.ldy; a.In = p.X; a.ldi = p.ldx; a.M = p.M; a.K = p.n_out; a.N = p.n_in; a.alpha = p.alpha;
    a.dW = p.dW; a.ldw = p.n_in; a.dW3 = p.dW3; a.tab = p.tab; a.tab_cols = p.tab_cols; a.tab_stride = p.tab_cols;
    return a;
}
inline ThinDgradArgs thin_dgrad_args(const Product& p) {
    ThinDgradArgs a{};
    a.D = p.Y; a.ldd = p.ldy; a.W = p.W; a.W3 = p.W3; a.ldw = p.n_in; a.C = p.dX; a.ldc = p.lddx; a.M = p.M; a.K = p.n_out; a.N = p.n_cols;
    a.accumulate = p.accumulate ? 1 : 0; a.alpha = p.alpha; a.ez = p.below.z; a.eld = p.below.ld; a.etab = p.below.tab; a.emu = p.below.mu; a.eistd = p.below.istd; a.stats = p.below.sums;
    return a;
}
inline GemmX gemm_fwd_x(const Product& p) {
    GemmX x{};
    x.n_tiles = (p.n_out + 31) / 32; x.ksteps = (p.n_in + 15) / 16;
    x.W = p.W; x.w_rows = p.n_out; x.w_cols = p.n_in; x.w_transpose = 0;      // split by the launcher, in its kernel's fragment order
    x.A = p.X; x.frag = p.frag; x.C = p.Y; x.M = p.M; x.N = p.n_out; x.K = p.n_in; x.lda = p.ldx; x.ldc = p.ldy;
    x.alpha = p.alpha; x.bias = p.bias; x.stats = p.stats; x.accumulate = 0;
    x.act_tab = p.tab; x.act_cols = p.tab_cols; x.a_padded = (p.x_padded && p.ldx >= (int64_t)x.ksteps * 16) ? 1 : 0;
    return x;
}
inline GemmX gemm_dgrad_x(const Product& p) {
    GemmX x{};
    x.n_tiles = (p.n_cols + 31) / 32; x.ksteps = (p.n_out + 15) / 16;
    x.W = p.W; x.w_rows = p.n_out; x.w_cols = p.n_in; x.w_transpose = 1;      // Bt[n = input feature][k = output feature] = W[k][n]: transposed split
    x.A = p.Y; x.frag = p.frag; x.C = p.dX; x.M = p.M; x.N = p.n_cols; x.K = p.n_out; x.lda = p.ldy; x.ldc = p.lddx;
    x.alpha = p.alpha; x.bias = nullptr; x.accumulate = p.accumulate ? 1 : 0;      // with `accumulate` and an epilogue the caller guarantees this is the last producer
    x.stats = p.below.sums; x.ez = p.below.z; x.eld = p.below.ld; x.etab = p.below.tab; x.emu = p.below.mu; x.eistd = p.below.istd;
    return x;
}
inline GemmArgs gemm_fwd_args(const Product& p) {
    GemmArgs g{};
    g.A = p.X; g.B = p.W; g.C = p.Y; g.M = p.M; g.N = p.n_out; g.K = p.n_in; g.sAm = p.ldx; g.sAk = 1; g.sBk = 1; g.sBn = p.n_in; g.ldc = p.ldy;
    g.alpha = p.alpha; g.bias = p.bias; g.colsum = p.colsum; g.flags = 0; g.splitk = 1;
    return g;
}
inline GemmArgs gemm_dgrad_args(const Product& p) {
    GemmArgs g{};
    g.A = p.Y; g.B = p.W; g.C = p.dX; g.M = p.M; g.N = p.n_cols; g.K = p.n_out; g.sAm = p.ldy; g.sAk = 1; g.sBk = p.n_in; g.sBn = 1; g.ldc = p.lddx;
    g.alpha = p.alpha; g.bias = nullptr; g.colsum = nullptr; g.flags = p.accumulate ? GEMM_ACCUM : 0; g.splitk = 1;
    return g;
}
inline GemmArgs gemm_wgrad_args(const Product& p) {      // split over the point dimension, fp32 atomics
    GemmArgs g{};
    g.A = p.Y; g.B = p.X; g.C = p.dW; g.M = p.n_out; g.N = p.n_in; g.K = p.M; g.sAm = 1; g.sAk = p.ldy; g.sBk = p.ldx; g.sBn = 1; g.ldc = p.n_in;
    g.alpha = p.alpha; g.bias = nullptr; g.colsum = nullptr; g.flags = GEMM_ATOMIC;
    g.splitk = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (p.M + 2047) / 2048));
    return g;
}

// ---- routing.  Thin: a head with at most four outputs as a stream over its input (thin_fwd / thin_wgrad / thin_dgrad_kernel), exact fp32;
// Rows: error-compensated bf16x3 (row GEMM for forward and dgrad, launch_wgrad_bf16x3); Fp32: exact-fp32 MFMA GEMM
enum class Route { Thin, Rows, Fp32 };
// a thin head: few outputs and enough rows that a stream beats a 32-column MFMA tile of which one to four columns are real
inline bool thin_head(const Product& p) { return p.n_out <= 4 && p.M >= 1024; }
// bf16x3 row-owner kernel usable for an [M x K] x [K x N] product (narrow N included: the kernels mask partial tiles)?  bf16x3 weight-gradient kernel used?
inline bool rows_ok(const Policy& pol, int64_t M, int K, int N) { return pol.bf16x3 && M >= pol.rows_min && K >= 1 && N >= 1 && gemm_rows_group_tiles((K + 15) / 16) > 0; }
inline bool wgrad_rows_ok(const Policy& pol, int64_t M) { return pol.bf16x3 && M >= pol.rows_min; }

inline Route route_fwd(const Product& p, const Policy& pol) {      // (the stream always adds a bias and has no statistics epilogue)
    if (pol.thin_fwd && switches().fused_heads && pol.bf16x3 && thin_head(p) && p.bias && !p.stats && thin_fwd_ok(thin_fwd_args(p))) return Route::Thin;
    return rows_ok(pol, p.M, p.n_in, p.n_out) ? Route::Rows : Route::Fp32;
}
inline Route route_dgrad(const Product& p, const Policy& pol) {
    const bool on = p.W3 ? switches().fused_heads : switches().thin_dgrad;      // the two-head form has its own switch
    if (pol.thin_dgrad && on && pol.bf16x3 && thin_head(p) && thin_dgrad_ok(thin_dgrad_args(p))) return Route::Thin;
    return rows_ok(pol, p.M, p.n_out, p.n_cols) ? Route::Rows : Route::Fp32;
}
inline Route route_wgrad(const Product& p, const Policy& pol) {
    const bool on = p.W3 ? switches().fused_heads : switches().thin_wgrad;
    if (on && !p.bn && pol.bf16x3 && thin_head(p) && thin_wgrad_ok(thin_wgrad_args(p))) return Route::Thin;
    return wgrad_rows_ok(pol, p.M) ? Route::Rows : Route::Fp32;
}
// ---- launching a routed product (the two-head form: Route::Thin only).  What a route cannot do is an error, never another route.
// Test introspection (rows_debug.h): a Thin / Fp32 route is recorded here, a Rows plan by launch_gemm_bf16x3; true = dry run, launch nothing.
inline bool route_noted_dry(Route r) {
    if (r != Route::Rows && rows_noting()) rows_note_route((int)r);
    return r != Route::Rows && rows_dry_run();
}
inline hipError_t run_fwd(const Product& p, Route r, hipStream_t st) {
    if (r == Route::Rows) return launch_gemm_bf16x3(gemm_fwd_x(p), st);
    if (r == Route::Fp32 && (p.tab || p.stats)) return hipErrorInvalidValue;      // activation on load / epilogue statistics need the row kernel
    if (route_noted_dry(r)) return hipSuccess;
    if (r == Route::Thin) return launch_thin_fwd(thin_fwd_args(p), st);
    return launch_gemm(gemm_fwd_args(p), st);
}
// the epilogue (p.below) is applied on the thin and row routes, ignored by the fp32 GEMM: the caller asks `r != Route::Fp32`
inline hipError_t run_dgrad(const Product& p, Route r, hipStream_t st) {
    if (r == Route::Rows) return launch_gemm_bf16x3(gemm_dgrad_x(p), st);
    if (route_noted_dry(r)) return hipSuccess;
    if (r == Route::Thin) return launch_thin_dgrad(thin_dgrad_args(p), st);
    return launch_gemm(gemm_dgrad_args(p), st);
}
inline hipError_t run_wgrad(const Product& p, Route r, hipStream_t st) {
    if (r == Route::Thin) return launch_thin_wgrad(thin_wgrad_args(p), st);
    if (r == Route::Rows) {
        const int64_t ldw = p.lddw ? p.lddw : p.n_in;
        if (p.bn && p.n_in > 256) {
            // The BatchNorm dZ pass (engine only) rides in the kernel for one block column over the inputs (in-place dZ): a layer with more than 256 inputs (fc5: [fc4 | PE]) goes as two
            // launches, the first 256 input columns with the dZ pass, then the rest on the finished dZ.  Each launch gets its window of the activation-on-load table ([a | b], b at distance tc).
            const int n0 = 256, tc = p.tab_cols;
            hipError_t e = launch_wgrad_bf16x3(p.Y, p.ldy, p.X, p.ldx, p.M, p.n_out, n0, p.alpha, p.dW, ldw, st, p.tab, tc < n0 ? tc : n0, p.bn, tc);
            if (e != hipSuccess) return e;
            const int rest = tc > n0 ? tc - n0 : 0;
            return launch_wgrad_bf16x3(p.Y, p.ldy, p.X + n0, p.ldx, p.M, p.n_out, p.n_in - n0, p.alpha, p.dW + n0, ldw, st, rest ? p.tab + n0 : nullptr, rest, nullptr, tc);
        }
        return launch_wgrad_bf16x3(p.Y, p.ldy, p.X, p.ldx, p.M, p.n_out, p.n_in, p.alpha, p.dW, ldw, st, p.tab, p.tab_cols, p.bn);
    }
    if (p.bn || p.tab) return hipErrorInvalidValue;
    return launch_gemm(gemm_wgrad_args(p), st);
}

}  // namespace snerf
