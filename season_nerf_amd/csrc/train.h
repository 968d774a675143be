// Layer-wise training engine (internal header): kernels' argument blocks and launchers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snerf {

enum GemmFlags : int { GEMM_ACCUM = 1, GEMM_ATOMIC = 2 };

struct GemmArgs {
    const float* A;
    const float* B;
    float* C;
    int64_t M, N, K;
    int64_t sAm, sAk, sBk, sBn, ldc;
    float alpha;
    const float* bias;    // [N] added before alpha (only by split 0)
    float* colsum;        // [N] += column sums of the written values (BatchNorm mean)
    int flags;
    int splitk;           // >1: K split over blockIdx.z, results combined with fp32 atomics (C must be zeroed)
};
hipError_t launch_gemm(const GemmArgs& g, hipStream_t st);

// bf16x3 row-owner GEMM (forward and dgrad of the training engine): C (+)= alpha*(A Bt^T + bias); Bt pre-split into MFMA
// fragment order by split_weights_kernel (gemm_rows.h; n_tiles x ksteps fragments of 2 KiB: bf16 hi, bf16 lo)
struct GemmX {
    const float* A;            // [M, lda] fp32, k contiguous
    // weights: either already split (frag, 32x32x16 fragment order: [n_tiles][ksteps][2][512] bf16) or raw fp32 (W != NULL): the
    // launcher then splits them into `frag` (scratch of n_tiles * ksteps * 2 KiB, any of the two fragment orders) for the kernel it picks
    const uint16_t* frag;
    const float* W;            // optional raw weights [w_rows, w_cols]; Bt[n][k] = W[n][k] (w_transpose = 0) or W[k][n] (1)
    int w_rows, w_cols, w_transpose;
    float* C;
    int64_t M, N, K, lda, ldc;
    int n_tiles, ksteps;       // ceil(N/32), ceil(K/16)
    float alpha;
    const float* bias;
    double* stats;             // optional [2][N]: += sum_m (v - alpha*bias), += sum_m (v - alpha*bias)^2   (train-mode BatchNorm)
    int accumulate;
    int reverse;               // row tiles from the last to the first (set by the launcher for gemm_rows16_kernel, see run_gemm_rows)
    const float* act_tab;      // optional activation-on-load table [a | b] x act_cols for the leading columns of A: sin(2 pi (a z + b))
    int act_cols;              // multiple of 8, <= K
    int tab_lds;               // set by the launcher: the table fits in LDS behind the weights
    // activation-backward epilogue (dgrad): C = dL/dH of the SineLayer below -> written as dL/d(arg) = C * cos(2 pi (a z + b));
    // ez = that layer's pre-activation [M, eld], etab = its [a | b] table (N columns), emu/eistd = its BatchNorm statistics
    // (NULL without BatchNorm); stats (required) receives sum v and sum v*xhat per column
    const float* ez;
    int64_t eld;
    const float *etab, *emu, *eistd;
    int a_padded;              // caller's promise: columns K .. 16*ksteps-1 of A exist (lda covers them) and hold zeros
};
int gemm_rows_group_tiles(int ksteps);      // 0 = K too large for the LDS-resident weight layout (caller falls back to fp32 MFMA)
hipError_t launch_gemm_bf16x3(const GemmX& g, hipStream_t st);      // routing, split and the launchers of the three translation units: gemm_rows.h
// gemm_areg.hip: N = 256 / 512 with the accumulators in AGPRs, A and the weights streamed (the reference's default width): the shapes it takes
bool gemm_areg_ok(const GemmX& g);
// bf16x3 weight gradient: dW[n_out, n_in] (ld ldw) += alpha * dZ[M, n_out]^T In[M, n_in]   (fp32 atomics over M-chunks)
// optional BatchNorm backward folded into the weight-gradient kernel (dZ holds dL/dY on entry, dL/dZ on exit; needs n_in <= 256)
struct WgradBN {
    const float* z;            // pre-activation of this layer [M, ldz]
    int64_t ldz;
    const float *gamma, *mu, *istd, *sdy, *sdyx;
    float inv_m;               // 1 / rows of the (global) batch the means were taken over
    float bias_alpha;
    float* dbias;              // += bias_alpha * sum_m dZ
};
int stream_direction(int64_t rows, bool take_turn = true);      // 0 / 1, alternating per large streaming launch (gemm.hip); !take_turn: the next launch's, left to it
// per-thread launch context of a training pass: the trainer's wgrad partial-sum scratch and its launch parity (nullptr / 0: none)
void gemm_launch_context(float* wgrad_partial, size_t wgrad_floats, unsigned* parity);
size_t gemm_wgrad_partial_floats();      // floats the two-stage weight-gradient reduction needs at most (grid blocks x 8 x 8 x 1024)
hipError_t launch_wgrad_bf16x3(float* dZ, int64_t ldz, const float* In, int64_t ldi, int64_t M, int n_out, int n_in, float alpha,
                               float* dW, int64_t ldw, hipStream_t st, const float* in_tab = nullptr, int in_cols = 0,
                               const WgradBN* bn = nullptr, int in_tab_stride = 0);      // in_tab_stride: see WgradX (0 = in_cols)
// ... as a plan and its execution (launch_wgrad_bf16x3 is the two in a row; plan_gemm_rows / run_gemm_rows are the row GEMMs' pair).  The plan launches
// nothing and reads no pointer: kernel = the TK_WGRAD_* instance, the workgroup's block of dW is 128 ta x 64 tb, the grid (bx, by, bz) = row blocks x
// blocks over n_out x blocks over n_in, partial = two-stage reduction through the partial-sum scratch (else atomics), reverse = stream_direction().
// take_turn = false: a plan for inspection - the direction is the one the next large launch will get, and that launch still gets it.
struct WgradPlan { int kernel, ta, tb; int64_t bx; int by, bz; int64_t rows_per_block; int partial, reverse; };
WgradPlan plan_wgrad_bf16x3(int64_t M, int n_out, int n_in, bool bn, bool take_turn = true);
hipError_t run_wgrad_bf16x3(const WgradPlan& p, float* dZ, int64_t ldz, const float* In, int64_t ldi, int64_t M, int n_out, int n_in, float alpha,
                            float* dW, int64_t ldw, hipStream_t st, const float* in_tab, int in_cols, const WgradBN* bn, int in_tab_stride);

// ---- elementwise / reduction kernels of the training path (train_kernels.hip)
// The kernel a launcher runs, as the test hook snerf_train_kernel_debug returns it (include/season_nerf_hip.h documents the numbers).  Where a launcher
// chooses between kernels, the *_choice function below IS its decision: the launcher branches on it and the hook reports it.
enum TrainKernel : int {
    TK_PE_POINTS = 0, TK_PE_SMALL, TK_COLREDUCE, TK_COLPASS_VEC1, TK_COLPASS_VEC2, TK_COLPASS_VEC3, TK_COLPASS_VEC4, TK_BN_BWD2, TK_BN_FINALIZE,
    TK_BN_FINALIZE_SHIFTED, TK_ACT_SUMS_FINALIZE, TK_ACT_TABLE, TK_SIN_FWD, TK_SIN_FWD_VEC, TK_THIN_DGRAD, TK_THIN_DGRAD_ACT, TK_POINT_OUT_FWD,
    TK_POINT_OUT_BWD, TK_SOFTMAX, TK_SOFTMAX_BWD, TK_SIGMOID, TK_SIGMOID_BWD, TK_COLSUM, TK_COPY_COLS, TK_BCAST_ROWS, TK_REDUCE_ROWS, TK_FILL_ZERO,
    TK_COPY_F32, TK_FILL_ZERO_BYTES, TK_COPY_BYTES,
    // wgrad_bf16x3_kernel<FULL, BNZ, TA, TB> (gemm.hip): block shape TA x TB, _BN = BNZ; TK_WGRAD_FULL = <true, ., 2, 4>.  plan_wgrad_bf16x3 relies on the order.
    TK_WGRAD_1X2, TK_WGRAD_1X2_BN, TK_WGRAD_2X2, TK_WGRAD_2X2_BN, TK_WGRAD_1X4, TK_WGRAD_1X4_BN, TK_WGRAD_2X4, TK_WGRAD_2X4_BN, TK_WGRAD_FULL, TK_WGRAD_FULL_BN,
    TK_THIN_WGRAD, TK_THIN_WGRAD_ACT, TK_THIN_FWD, TK_THIN_FWD_ACT, TK_COUNT
};
struct PeArgs {            // positions (from rays or explicit) -> PE(pos) [N,64] (63 features + zero pad) and points [N,3]
    int64_t n;
    int n_samples;
    const float *points, *top, *bot, *tvals;
    float* pe;             // [N,64]
    float* pts;            // [N,3] or NULL
    float* pe2;            // optional second copy of PE with row stride ld2 (a concat buffer's columns), or NULL
    int64_t ld2;
};
hipError_t launch_pe_points(const PeArgs& a, hipStream_t st);
// per-row encodings of small vectors: sun [G,3] -> [G,28] (27 + pad), time[:,0:2] [G,4] -> [G,12] (10 + pad)
hipError_t launch_pe_small(const float* in, int in_stride, int n_dims, int n_freq, int64_t rows, float* out, int out_stride, hipStream_t st);

// column reductions over rows of X [M, ld] for C columns.  mode 0: sum (x - mu_c)^2 -> out0
// mode 1: dY = dH*cos(Y) with Y = g_c*(z - mu_c)*istd_c + b_c (written in place over dH), out0 += sum dY, out1 += sum dY*xhat
// mode 2: dZ = dH*cos(Z) in place, out0 += sum dZ            (layers without BatchNorm)
struct ColArgs {
    int mode;
    int64_t M;
    int C;
    int64_t ld;            // row stride of Z
    int64_t ldd;           // row stride of D (0 = same as ld)
    const float* Z;        // pre-activation [M, ld]
    float* D;              // gradient buffer [M, ldd] (in place)
    const float *mu, *istd, *gamma, *beta;
    float *out0, *out1;
    float alpha0;          // scale of the out0 accumulation (mode 2: 30 = d bias of the Linear)
    int64_t M_global;      // mode 3: rows of the global batch the BatchNorm means were taken over (>= M)
};
int colreduce_choice(const ColArgs& a);                  // TK_COLREDUCE, TK_COLPASS_VEC1 or TK_COLPASS_VEC2
int colpass_rows_per_block(int64_t M, int C);            // rows a block of colpass_vec_kernel walks (32..512)
hipError_t launch_colreduce(const ColArgs& a, hipStream_t st);
struct ThinDgradArgs {     // input gradient of a head with K <= 4 outputs as a stream over C (train_kernels.hip: thin_dgrad_kernel)
    const float* D;        // [M, ldd]: dL/d(head output), K leading columns
    const float* W;        // [K, ldw]: the head's weights (row k = output k)
    const float* W3;       // optional: row 3 lives here instead (two heads in one launch: colour rows 0..2, density row 3)
    float* C;              // [M, ldc], N columns
    int64_t M, ldd, ldw, ldc;
    int K, N, accumulate;
    float alpha;
    // optional activation backward of the layer below (as the row GEMMs' epilogue): pre-activations, [a | b] table (N each), BatchNorm
    // mean / istd (or NULL), the double column sums [2][N]
    const float* ez;
    int64_t eld;
    const float *etab, *emu, *eistd;
    double* stats;
};
bool thin_dgrad_ok(const ThinDgradArgs& a);
int thin_dgrad_choice(const ThinDgradArgs& a);           // TK_THIN_DGRAD or TK_THIN_DGRAD_ACT
int thin_dgrad_rows_per_block(int64_t M, int N);         // rows of a chunk of thin_dgrad_kernel (32..256)
hipError_t launch_thin_dgrad(const ThinDgradArgs& a, hipStream_t st);
struct ThinFwdArgs {       // forward of heads with K <= 4 outputs in all as one stream over their common input (train_kernels.hip: thin_fwd_kernel)
    const float* In;       // [M, ldi], N columns (the first tab_cols of them stored as pre-activations: activation on load)
    const float* W;        // [K, ldw] rows 0..K-1 - row 3 at W3 if set (colour head rows 0..2, density head row 3)
    const float* W3;
    const float* bias;     // [K] - element 3 at bias3 if set
    const float* bias3;
    float* Out;            // [M, ldo]: Out[m, k] = alpha * (sum_n In[m, n] W[k, n] + bias[k])
    int64_t M, ldi, ldw, ldo;
    int K, N;
    float alpha;
    const float* tab;
    int tab_cols, tab_stride;
};
bool thin_fwd_ok(const ThinFwdArgs& a);
inline int thin_fwd_choice(const ThinFwdArgs& a) { return (a.tab && a.tab_cols > 0) ? TK_THIN_FWD_ACT : TK_THIN_FWD; }            // thin_fwd_kernel<true / false>
hipError_t launch_thin_fwd(const ThinFwdArgs& a, hipStream_t st);
struct ThinWgradArgs {     // weight gradient of a head with K <= 4 outputs as a stream over its input (train_kernels.hip: thin_wgrad_kernel)
    const float* D;        // [M, ldd]: dL/d(head output), K leading columns
    const float* In;       // [M, ldi], N columns: the head's input - or, for the first tab_cols columns, its stored pre-activation (activation on load)
    float* dW;             // [K, ldw] += alpha * D^T In  (two stages: per-block sums in `partial`, then one reduction kernel - deterministic)
    float* partial;        // [blocks, K * N] scratch (set by the launcher)
    float* dW3;            // optional: row 3 of the result goes here instead (two heads in one launch)
    int64_t M, ldd, ldi, ldw;
    int K, N;
    float alpha;
    const float* tab;      // optional [a | b] table: In[:, c] = sin(2 pi (a[c] z + b[c])) for c < tab_cols, b at distance tab_stride
    int tab_cols, tab_stride;
};
float* gemm_partial_scratch(hipStream_t st, size_t floats);      // gemm.hip: the calling trainer's pre-carved partial-sum scratch (or the stream's own)
bool thin_wgrad_ok(const ThinWgradArgs& a);
inline int thin_wgrad_choice(const ThinWgradArgs& a) { return (a.tab && a.tab_cols > 0) ? TK_THIN_WGRAD_ACT : TK_THIN_WGRAD; }      // thin_wgrad_kernel<true / false>
hipError_t launch_thin_wgrad(const ThinWgradArgs& a, hipStream_t st);

// BatchNorm finalize: mean = sum/M, var = m2/M, istd; EMA of running stats (momentum 0.01, unbiased var)
hipError_t launch_bn_finalize(const float* colsum, const float* m2, int64_t M, int C, float* mean, float* istd,
                              float* running_mean, float* running_var, int stage, hipStream_t st);
// H = sin(gamma*(Z-mu)*istd + beta) (bn) or sin(Z)
// consumes AND clears the sums; tab (optional): the layer's activation-on-load table [a | b] from gamma / beta and the new statistics
hipError_t launch_bn_finalize_shifted(double* stats, const float* bias, float alpha, int64_t M, int C, float* mean, float* istd,
                                      float* running_mean, float* running_var, const float* gamma, const float* beta, float* tab,
                                      hipStream_t st);
int sin_fwd_choice(const float* Z, const float* H, int C, int64_t ldz, int64_t ldh);      // TK_SIN_FWD or TK_SIN_FWD_VEC
hipError_t launch_sin_fwd(const float* Z, float* H, int64_t M, int C, int64_t ldz, int64_t ldh, const float* mu, const float* istd,
                          const float* gamma, const float* beta, hipStream_t st);
// BN backward second pass: dZ = gamma*istd*(dY - sdy/M - xhat*sdyx/M) in place; colsum(dZ) -> out (bias grad)
int bn_bwd2_choice(const float* Z, const float* D, int C, int64_t ld, int64_t ldd, bool d_is_dy);      // TK_BN_BWD2, TK_COLPASS_VEC3 or TK_COLPASS_VEC4
hipError_t launch_bn_bwd2(const float* Z, float* D, int64_t M, int C, int64_t ld, int64_t ldd, const float* mu, const float* istd,
                          const float* gamma, const float* beta, const float* sdy, const float* sdyx, float* dbias_sum, float alpha,
                          int64_t M_global, hipStream_t st, bool d_is_dy = false);
hipError_t launch_act_sums_finalize(double* stats, int C, float scale0, float* out0, float* out1, float* acc0, float* acc1, hipStream_t st);      // consumes and clears the sums
// activation-on-load table of a SineLayer: dst = [a | b] (n each), a = gamma*istd/(2 pi), b = (beta - gamma*mu*istd)/(2 pi);
// all-NULL statistics = a layer without BatchNorm (a = 1/(2 pi), b = 0)
hipError_t launch_act_table(const float* mu, const float* istd, const float* gamma, const float* beta, int n, float* dst, hipStream_t st);

// point outputs: rho = softplus(head[:,3]), col = sigmoid(head[:,0:3] + sum_c cls[g,c]*adj[:,c,:]), sv = sigmoid(sv_raw)
struct PointOutArgs {
    int64_t n;
    int n_samples, C;
    const float *head, *adj, *sv_raw, *cls;     // [N,4], [N,3C], [N], [R,C]
    float *rho, *col, *sv;                      // [N], [N,3], [N]
    float* adjust_col;                          // [N,3] optional: sum_c cls*adj
    // backward (all optional): d_rho [N], d_col [N,3] -> d_head [N,4], d_adj [N,3C], d_cls [R,C] (atomic), d_sv -> d_sv_raw
    const float *d_rho, *d_col, *d_sv;
    float *d_head, *d_adj, *d_cls, *d_sv_raw;
};
hipError_t launch_point_out(const PointOutArgs& a, bool backward, hipStream_t st);

// compositing backward (one wave per ray): from dL/dRendered_Col, dL/dAlbedo, dL/dPE (optional) -> d_rho, d_col, d_sky
struct CompBwdArgs {
    int64_t n_rays;
    int n_samples;
    const float *top, *bot;
    const float *rho, *col, *sv, *sky;          // forward inputs ([N], [N,3], [N], [R,3])
    const float *g_rgb, *g_albedo, *g_pe;       // [R,3] or NULL, [R,3] or NULL, [N] or NULL
    // DSM-prior phase (Eval_Tools_2.py:218-248): merged density rho*trust + rho_prior*(1-trust); gradients of
    // Rendered_Col_Merged / merged Albedo_Color.  The solar factor always comes from the un-merged PS.
    const float* rho_prior;                     // [N] or NULL
    float trust;
    const float* trust_dev;                     // optional device-resident trust (captured steps); overrides `trust`
    const float *g_rgb_m, *g_albedo_m;          // [R,3] or NULL
    float *d_rho, *d_col, *d_sky;               // [N], [N,3], [R,3] (d_sky is overwritten)
    // classic solar model (Solar_Type_2, Eval_Tools_2.py:211-212): Rendered_Col = sum PS*Col*(SV + (1-SV)*Sky) per sample;
    // the solar visibility then carries gradient: d_sv [N] (required when classic != 0)
    int classic;
    float* d_sv;
};
hipError_t launch_composite_bwd(const CompBwdArgs& a, hipStream_t st);

// softmax rows [R,C] forward / backward; sigmoid forward/backward on small tensors
hipError_t launch_softmax(const float* logits, float* p, int64_t rows, int C, hipStream_t st);
hipError_t launch_softmax_bwd(const float* p, const float* dp, float* dlogits, int64_t rows, int C, hipStream_t st);
hipError_t launch_sigmoid(const float* x, float* y, int64_t n, hipStream_t st);
hipError_t launch_sigmoid_bwd(const float* y, const float* dy, float* dx, int64_t n, hipStream_t st);
// column sum of a small-N matrix [M,C] (bias gradients of head layers): out[c] += alpha * sum_m X[m,c]
hipError_t launch_colsum(const float* X, int64_t M, int C, int64_t ld, float alpha, float* out, hipStream_t st);
// concat-free helpers
hipError_t launch_copy_cols(const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int64_t M, int C, bool accumulate, hipStream_t st);
hipError_t launch_fill_zero_bytes(void* p, size_t bytes, hipStream_t st);
hipError_t launch_copy_bytes(void* d, const void* s, size_t bytes, hipStream_t st);
hipError_t launch_copy_f32(float* d, const float* s, int64_t n, hipStream_t st);            // the engine's device-to-device copy and zero-fill: kernels, so that a
hipError_t launch_fill_zero(float* p, int64_t n, hipStream_t st);                          // captured step holds no hipGraph memory-operation node (train.cpp)
hipError_t launch_round_bf16(float* p, int64_t ld, int64_t M, int C, hipStream_t st);      // experiment switch SNERF_TRAIN_DY_BF16 only
// broadcast per-group rows [G,C] to per-point rows [G*S, C] and the transposed reduction
hipError_t launch_bcast_rows(const float* src, int C, float* dst, int64_t ld_dst, int col0, int64_t n, int n_samples, hipStream_t st);
hipError_t launch_reduce_rows(const float* src, int64_t ld_src, int col0, int C, float* dst, int64_t n_groups, int n_samples, hipStream_t st);
// the scalar loss terms of get_loss (solar rays, default solar model) and their gradients: MSE or Barron's adaptive colour loss, without or with the
// DSM-prior phase, with the weight vector and the gradients of the loss objects' alpha and scale (train_kernels.hip, snerf_loss_all_* of include/season_nerf_hip.h)
constexpr int kLossAdaptive = 1, kLossPrior = 2, kLossSkyDetached = 4;
struct LossAllArgs {
    int64_t R, Rs;                                          // image rays, sun rays
    int S, flags;
    const float *rgb, *rgb_merged, *gt, *albedo, *sky;      // [R,3] (sky: per ray, after the sigmoid); rgb_merged optional: what `Color` is formed on
    const float *sv, *pv, *pe_sun;                          // sun-ray pass [Rs,S]
    const float *pe, *pe_sup;                               // prior: PE, PE_Supervised of the image rays [R,S]
    const float *alpha_c, *scale_c, *alpha_a, *scale_a;     // adaptive: the colour loss object's alpha / scale [3]; adaptive + prior: the alpha loss object's [1]
    const double *logz_v, *logz_s;                          // adaptive: log Z table, values and slopes [513], float64 (see ada_logz)
    const float* alb_min_in;                                // optional [3]: the albedo minimum over the GLOBAL batch (data parallel); NULL: the local one
    int world;                                              // ranks the global batch spans (1 without alb_min_in)
    float w_sc, w_color, w_alpha;                           // weights of the Solar_Correction family, Color / Color_ada, Alpha_Adjust / Alpha_Adjust_ada
};
struct LossAllIdx { int sc, sc2, sky, alb, aa_ada, c_ada, c_alpha, c_width, aa, a_alpha, a_width, color, n; };      // position of each term in the value vector (-1: absent)
struct LossAllGrads { float *d_rgb, *d_rgb_merged, *d_albedo, *d_sky, *d_sv, *d_pe, *d_alpha_c, *d_scale_c, *d_alpha_a, *d_scale_a; };
#if defined(__HIPCC__)
__host__ __device__
#endif
inline LossAllIdx loss_all_idx(int flags) {      // the key order training.get_loss produces (Eval_Tools_2.py:361-450)
    LossAllIdx I{0, 1, 2, 3, -1, -1, -1, -1, -1, -1, -1, -1, 0};
    const bool ada = flags & kLossAdaptive, prior = flags & kLossPrior;
    int n = 4;
    if (!ada) { I.color = n++; if (prior) I.aa = n++; }
    else {
        if (prior) I.aa_ada = n++;
        I.c_ada = n++; I.c_alpha = n++; I.c_width = n++;
        if (prior) { I.aa = n++; I.a_alpha = n++; I.a_width = n++; }
        I.color = n++;
    }
    I.n = n;
    return I;
}
size_t loss_all_scratch_bytes();
hipError_t launch_loss_all(const LossAllArgs& a, void* scratch, float* vals, float* wts, float* aux14, hipStream_t st);
hipError_t launch_loss_all_bwd(const LossAllArgs& a, const float* g, const float* aux14, const LossAllGrads& G, hipStream_t st);
hipError_t launch_adam_dev(float* params, const float* grads, float* m, float* v, int64_t n, const float* d_hyper6, hipStream_t st);
// Adam on a flat arena (torch.optim.Adam semantics, no weight decay)
hipError_t launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2, float eps, int step, hipStream_t st);

}  // namespace snerf
