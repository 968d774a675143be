// Layer-wise training engine: forward with batch-statistics BatchNorm (+ running-stat EMA), backward, Adam.
// Reference semantics: T_NeRF.forward / forward_Solar in .train() mode (T_NeRF_net_v2.py:75-157, misc.py:148-189),
// Eval_Tools_2.py:165-215 (compositing) and :297-337 (sun-ray pass, trunk under no_grad), mg_run_NeRF.py:288-326.
// The caller (PyTorch) owns every buffer: parameter / gradient / Adam arenas and the activation workspace.
#include "../../include/season_nerf_hip.h"

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <mutex>
#include <set>
#include <vector>

#include "kernels.h"
#include "linear_product.h"
#include "train.h"

// Every device-to-device copy and zero-fill of the engine is a KERNEL of ours, never hipMemcpyAsync / hipMemsetAsync.  Inside a captured training step a
// runtime memory operation becomes a hipGraph MEMCPY / MEMSET node, and on ROCm 7.2 (graph nodes recorded as AQL packets, DEBUG_CLR_GRAPH_PACKET_CAPTURE
// default on) replays of a graph that holds such nodes computed garbage once eager work of the same process (a save point's validation, a second capture)
// had run between them: gradients of 1e5..1e36 in whole layers, Adam moments to match - the failure family rounds 4-6 chased.  With kernel
// nodes only, 0 of 68 driver runs differ from the eager run; with the memory operations back (SNERF_TRAIN_MEMOPS=1, kept for the reproduction:
// tools/graph_wait_probe4.py) 29 of 29 do; with the memory operations AND packet capture off, 0 of 6.  The defect is the runtime's and reproduces without any
// code of this repository: tools/graph_memset_min.py (25 lines), profiles/r6/graph_memop_repro.txt.
static bool train_memops() { return snerf::switches().memops; }
static hipError_t snerf_zero_async(void* p, int value, size_t bytes, hipStream_t st) {
    if (train_memops()) return hipMemsetAsync(p, value, bytes, st);
    if (value != 0) return hipErrorInvalidValue;                     // (the engine only ever zeroes)
    if (bytes % 4 != 0 || ((uintptr_t)p & 3)) return snerf::launch_fill_zero_bytes(p, bytes, st);
    return snerf::launch_fill_zero((float*)p, (int64_t)(bytes / 4), st);
}
static hipError_t snerf_copy_async(void* d, const void* s_, size_t bytes, hipStream_t st) {
    if (train_memops()) return hipMemcpyAsync(d, s_, bytes, hipMemcpyDeviceToDevice, st);
    if (bytes % 4 != 0 || (((uintptr_t)d | (uintptr_t)s_) & 3)) return snerf::launch_copy_bytes(d, s_, bytes, st);
    return snerf::launch_copy_f32((float*)d, (const float*)s_, (int64_t)(bytes / 4), st);
}

using namespace snerf;

extern int snerf_set_error(int code, const std::string& msg);   // api.cpp

namespace {

struct LayerP {
    std::string name;
    int n_out, n_in;
    bool sine, bn;
    int64_t w, b, g, beta;     // offsets (floats) in the parameter arena; g/beta only with bn
    int64_t rm, rv;            // offsets in the buffer arena (running mean/var); only with bn
};

enum L {
    L_FC1, L_FC2, L_FC3, L_FC4, L_FC5, L_FC6, L_FC7, L_FC8, L_FC9, L_COL, L_SIG, L_S1, L_S2, L_S3, L_S4, L_K1, L_K2,
    L_T1, L_T2, L_CL, L_A1, L_A2, L_A3, L_AC, L_DEAD0, L_DEAD1, L_DEAD2, L_NUM
};

struct Act {           // a [rows, cols] fp32 matrix inside the workspace
    float* p = nullptr;
    int64_t ld = 0;
    // activation on load: when tab != nullptr the first `cols` columns hold the PRE-activation of a SineLayer and every
    // consumer (row GEMM, wgrad) applies sin(2 pi (a z + b)) with tab = [a | b] while loading - the post-activation is not stored
    const float* tab = nullptr;
    int cols = 0;
    // the columns between the layer's n_in and the next multiple of 16 exist and hold zeros (row GEMM: no K tail to guard)
    bool padded = false;
};

}  // namespace

struct snerf_trainer {
    int W, C, W2, W4;
    std::vector<LayerP> layers;
    int64_t n_params = 0, n_buffers = 0;
    float *params = nullptr, *grads = nullptr, *adam_m = nullptr, *adam_v = nullptr, *buffers = nullptr;
    char* ws = nullptr;
    size_t ws_bytes = 0;
    // state of the last forward passes (needed by backward)
    int64_t R = 0, Rs = 0;
    int S = 0;
    int img_flags = 0;                              // flags of the last image-pass forward (bit 0: classic solar model)
    // workspace carve (set by carve())
    struct Pass {
        int64_t R = 0, N = 0;
        Act E, In5, Z[9], H[9], head, Za[3], Ha[3], adj, In_s1, Zs[3], Hs[3], sv_raw, tmpA, tmpB;
        float *pts, *rho, *col, *sv, *pe_sun, *pe_time, *Zt1, *Ht1, *Zt2, *Ht2, *logits, *cls, *Zk1, *Hk1, *sky_raw, *sky;
        float* bn;             // [8 layers][4][W]: colsum, m2, mean, istd
        float *top, *bot, *tvals;   // engine-owned copies: the caller's tensors may be recycled before backward
        // what the consumers of each per-point SineLayer read: the materialised H, or (activation on load) Z + its table
        Act Hc[9], Hac[3], Hsc[3], In5c, In_s1c, Zc3, Zc8;
        float* tabs = nullptr;      // [15 layers][2][W] activation-on-load tables of this pass
        bool aol = false;
        bool batch_bn = true;       // the last forward of this pass normalised with batch statistics (train_bn != 0); false: with the running estimates
        float* tab(int slot, int W) const { return aol ? tabs + (int64_t)slot * 2 * W : nullptr; }      // slots: 0-8 trunk, 9-11 adjust, 12-14 solar
    } img, sol;
    Act dA, dB, dX1;
    float *d_head, *d_adj, *d_rho, *d_col, *d_sky, *d_cls, *d_sv_raw, *rayA, *rayB, *bn_bwd;   // bn_bwd: [2][W]
    uint16_t* w_frag = nullptr;                     // scratch: one weight matrix split into bf16 hi/lo MFMA fragments
    double* bn_stats = nullptr;                     // [2][W] shifted column sums from the GEMM epilogue
    int gemm_mode = 1;                              // 1 = bf16x3 MFMA for forward/dgrad (default), 0 = exact fp32 MFMA everywhere
    int aol_mode = 1;                               // 1 = activation on load where possible (SNERF_TRAIN_AOL=0: always store H)
    // data-parallel BatchNorm over the global batch: sum-all-reduce of the statistics buffers (snerf_trainer_set_allreduce)
    snerf_allreduce_fn ar_fn = nullptr;
    void* ar_user = nullptr;
    int world = 1;
    float* wgrad_partial = nullptr;                 // partial dW blocks of the two-stage weight-gradient reduction (carved: no hipMalloc in a step)
    size_t wgrad_partial_floats = 0;
    unsigned launch_parity = 0;                     // direction of the next streaming launch; reset at the start of every pass
};

// Every pass runs under its trainer's launch context (gemm.hip): the row direction of a streaming launch - and with it the summation order of the
// weight gradients' fp32 stages - depends on the launch's position in the pass only, and the partial sums land in this trainer's workspace.
struct CtxGuard {
    explicit CtxGuard(snerf_trainer* t) { t->launch_parity = 0; gemm_launch_context(t->wgrad_partial, t->wgrad_partial_floats, &t->launch_parity); }
    ~CtxGuard() { gemm_launch_context(nullptr, 0, nullptr); }
};

// sum the buffer over all ranks (no-op without a registered collective)
static int all_reduce(snerf_trainer* t, void* buf, int64_t count, bool is_double, hipStream_t st) {
    if (!t->ar_fn) return SNERF_OK;
    if (t->ar_fn(t->ar_user, buf, count, is_double ? 1 : 0, (void*)st) != 0)
        return snerf_set_error(SNERF_E_STATE, "the registered all-reduce callback failed");
    return SNERF_OK;
}

static int64_t align64(int64_t x) { return (x + 63) / 64 * 64; }

static void build_layers(snerf_trainer* t) {
    const int W = t->W, C = t->C, W2 = t->W2, W4 = t->W4;
    auto add = [&](const char* name, int n_out, int n_in, bool sine, bool bn) {
        LayerP l;
        l.name = name; l.n_out = n_out; l.n_in = n_in; l.sine = sine; l.bn = bn;
        l.w = t->n_params; t->n_params += (int64_t)n_out * n_in;
        l.b = t->n_params; t->n_params += n_out;
        l.g = l.beta = l.rm = l.rv = -1;
        if (bn) {
            l.g = t->n_params; t->n_params += n_out;
            l.beta = t->n_params; t->n_params += n_out;
            l.rm = t->n_buffers; t->n_buffers += n_out;
            l.rv = t->n_buffers; t->n_buffers += n_out;
        }
        t->layers.push_back(l);
    };
    add("G_NeRF_net.fc1", W, 63, true, false);
    add("G_NeRF_net.fc2", W, W, true, true);
    add("G_NeRF_net.fc3", W, W, true, true);
    add("G_NeRF_net.fc4", W, W, true, true);
    add("G_NeRF_net.fc5", W, W + 63, true, true);
    add("G_NeRF_net.fc6", W, W, true, true);
    add("G_NeRF_net.fc7", W, W, true, true);
    add("G_NeRF_net.fc8", W, W, true, true);
    add("G_NeRF_net.fc9", W2, W, true, true);
    add("G_NeRF_net.fc10Col", 3, W2, false, false);
    add("G_NeRF_net.fc10Sigma", 1, W2, false, false);
    add("G_NeRF_net.fc_solar_1", W2, W2 + 27, true, false);
    add("G_NeRF_net.fc_solar_2", W2, W2, true, false);
    add("G_NeRF_net.fc_solar_3", W2, W2, true, false);
    add("G_NeRF_net.fc_solar_4", 1, W2, false, false);
    add("G_NeRF_net.fc_sky_color_1", W4, 27, true, false);
    add("G_NeRF_net.fc_sky_color_2", 3, W4, false, false);
    add("time_layer_1", W, 10, true, false);
    add("time_layer_2", W, W, true, false);
    add("get_class_layer", C, W, false, false);
    add("adjust_layer_1", W, W2, true, false);
    add("adjust_layer_2", W, W, true, false);
    add("adjust_layer_3", W, W, true, false);
    add("adjust_col", 3 * C, W, false, false);
    add("adjust_rho", C, W, false, false);            // dead heads: parameters only (never used, never get a gradient)
    add("adjust_solar_vis", C, W, false, false);
    add("adjust_sky_col", 3 * C, W, false, false);
}

// ---- workspace carving ------------------------------------------------------------------------------
struct Carver {
    char* base;
    size_t off = 0;
    float* take(int64_t floats) {
        float* p = base ? (float*)(base + off) : nullptr;
        off += (size_t)align64(floats) * 4;
        return p;
    }
    Act mat(int64_t rows, int64_t ld) { Act a; a.p = take(rows * ld); a.ld = ld; return a; }
};

static size_t carve(snerf_trainer* t, char* base, int64_t R, int64_t Rs, int S) {
    Carver c{base};
    const int W = t->W, W2 = t->W2, W4 = t->W4, C = t->C;
    for (int pass = 0; pass < 2; ++pass) {
        snerf_trainer::Pass& P = pass == 0 ? t->img : t->sol;
        const int64_t Rr = pass == 0 ? R : Rs, N = Rr * S;
        P.R = Rr; P.N = N;
        P.E = c.mat(N, 64);
        P.In5 = c.mat(N, W + 64);
        for (int l = 0; l < 9; ++l) {
            const int w = l == 8 ? W2 : W;
            P.Z[l] = c.mat(N, w);
            if (l == 3) { P.H[l].p = P.In5.p; P.H[l].ld = W + 64; }     // fc4's output lives inside fc5's concat input
            else P.H[l] = c.mat(N, w);
        }
        P.head = c.mat(N, 4);
        for (int l = 0; l < 3; ++l) { P.Za[l] = c.mat(N, W); P.Ha[l] = c.mat(N, W); }
        P.adj = c.mat(N, 3 * C);
        P.In_s1 = c.mat(N, W2 + 32);         // [fc9 | PE(sun) 27 + 1 | 4 zero columns]: 16-column granules for the row GEMM
        for (int l = 0; l < 3; ++l) { P.Zs[l] = c.mat(N, W2); P.Hs[l] = c.mat(N, W2); }
        P.sv_raw = c.mat(N, 1);
        P.pts = c.take(N * 3); P.rho = c.take(N); P.col = c.take(N * 3); P.sv = c.take(N);
        P.pe_sun = c.take(Rr * 28); P.pe_time = c.take(Rr * 12);
        P.Zt1 = c.take(Rr * W); P.Ht1 = c.take(Rr * W); P.Zt2 = c.take(Rr * W); P.Ht2 = c.take(Rr * W);
        P.logits = c.take(Rr * C); P.cls = c.take(Rr * C);
        P.Zk1 = c.take(Rr * W4); P.Hk1 = c.take(Rr * W4); P.sky_raw = c.take(Rr * 3); P.sky = c.take(Rr * 3);
        P.bn = c.take(8 * 4 * W);
        P.top = c.take(Rr * 3); P.bot = c.take(Rr * 3); P.tvals = c.take(S);
        P.tabs = c.take(15 * 2 * W);
    }
    const int64_t Nmax = (R > Rs ? R : Rs) * S, Rmax = R > Rs ? R : Rs;
    t->dA = c.mat(Nmax, W + 64);
    t->dB = c.mat(Nmax, W + 64);
    t->dX1 = c.mat(Nmax, W2);
    t->d_head = c.take(Nmax * 4); t->d_adj = c.take(Nmax * 3 * C); t->d_rho = c.take(Nmax); t->d_col = c.take(Nmax * 3);
    t->d_sky = c.take(Rmax * 3); t->d_cls = c.take(Rmax * C); t->d_sv_raw = c.take(Nmax);
    t->rayA = c.take(Rmax * W); t->rayB = c.take(Rmax * W);
    t->bn_bwd = c.take(2 * W);
    const int64_t frag_bytes = (int64_t)((W + 64 + 31) / 32) * ((W + 64 + 15) / 16) * 2048;
    t->w_frag = (uint16_t*)c.take(frag_bytes / 4);
    t->bn_stats = (double*)c.take(4 * W + 2);
    t->wgrad_partial_floats = gemm_wgrad_partial_floats();
    t->wgrad_partial = c.take((int64_t)t->wgrad_partial_floats);
    return c.off;
}

// ---- building blocks ----------------------------------------------------------------------------------
#define HIPCK(x)                                                                                   \
    do {                                                                                           \
        hipError_t _e = (x);                                                                       \
        if (_e != hipSuccess) return snerf_set_error(SNERF_E_HIP, std::string(#x) + ": " + hipGetErrorString(_e)); \
    } while (0)
#define RC(x) do { int _rc = (x); if (_rc) return _rc; } while (0)

// ---- the engine's side of linear_product.h.  The engine as a caller: small (per-ray) batches go to exact fp32; `head`: a plain Linear (its forward may stream)
static Policy engine_policy(const snerf_trainer* t, bool head = false) { return Policy{t->gemm_mode == 1, 1024, head, true}; }
// layer L on input In; Y is its output (forward) or the gradient with respect to it (backward)
static Product product_of(const snerf_trainer* t, const LayerP& L, const Act& In, int64_t M, float* Y, int64_t ldy, float alpha) {
    Product p;
    p.M = M; p.n_in = L.n_in; p.n_out = L.n_out; p.alpha = alpha; p.W = t->params + L.w; p.bias = t->params + L.b; p.dW = t->grads + L.w;
    p.X = In.p; p.ldx = In.ld; p.tab = In.tab; p.tab_cols = In.tab ? In.cols : 0; p.x_padded = In.padded; p.Y = Y; p.ldy = ldy; p.frag = t->w_frag;
    return p;
}
// `below` (optional): the SineLayer whose output gradient a dgrad produces.  When that layer's [a | b] table exists (activation on load) and the dgrad covers
// all of its columns, its activation backward (x cos, column sums into t->bn_stats) happens in the dgrad's epilogue on the thin and row routes; the
// consumer then skips its own reduction sweep.
struct ActBelow { const LayerP* L; Act Z; const float* tab; float* bnslot; };
static Epilogue epilogue_of(const snerf_trainer* t, const ActBelow* below, int n_cols) {
    Epilogue e;
    if (!below || !below->tab || below->L->n_out != n_cols) return e;
    e.z = below->Z.p; e.ld = below->Z.ld; e.tab = below->tab; e.sums = t->bn_stats;
    if (below->L->bn) { e.mu = below->bnslot + 2 * t->W; e.istd = below->bnslot + 3 * t->W; }
    return e;
}

// Z[M, n_out] = alpha * (In[M, K] W^T + b);  colsum (fp32 route) / stats (row route) optional
static hipError_t linear_fwd(snerf_trainer* t, const LayerP& L, Act In, int64_t M, float* Z, int64_t ldz, float alpha, float* colsum, hipStream_t st, double* stats = nullptr, bool head = false) {
    Product p = product_of(t, L, In, M, Z, ldz, alpha);
    p.colsum = colsum; p.stats = stats;
    return run_fwd(p, route_fwd(p, engine_policy(t, head)), st);
}
// dIn[M, n_cols] (+)= alpha * dZ[M, n_out] W[:, :n_cols];  *fused reports that the epilogue of `below` was applied
static hipError_t linear_dgrad(snerf_trainer* t, const LayerP& L, float* dZ, int64_t ldz, int64_t M, float* dIn, int64_t ld_in, int n_cols, float alpha, bool accumulate, hipStream_t st,
                               const ActBelow* below = nullptr, bool* fused = nullptr) {
    Product p = product_of(t, L, Act{}, M, dZ, ldz, alpha);
    p.dX = dIn; p.lddx = ld_in; p.n_cols = n_cols; p.accumulate = accumulate; p.below = epilogue_of(t, below, n_cols);
    const Route r = route_dgrad(p, engine_policy(t));
    if (fused) *fused = p.below.z && r != Route::Fp32;
    return run_dgrad(p, r, st);
}
// dW[n_out, n_in] += alpha * dZ^T In;  bn (optional, needs wgrad_rows_ok): the BatchNorm dZ pass rides in the weight-gradient kernel
static hipError_t linear_wgrad(snerf_trainer* t, const LayerP& L, float* dZ, int64_t ldz, Act In, int64_t M, float alpha, hipStream_t st, const WgradBN* bn = nullptr) {
    Product p = product_of(t, L, In, M, dZ, ldz, alpha);
    p.bn = bn;
    return run_wgrad(p, route_wgrad(p, engine_policy(t)), st);
}

// SineLayer forward in train mode: Z = 30(In W^T + b) [stashed], H = sin(BN_batch(Z)) or sin(Z)
// tab_out != nullptr: activation on load - no sin pass; the layer's [a | b] table is written instead and H stays unwritten
static int sine_fwd(snerf_trainer* t, const LayerP& L, Act In, int64_t M, Act Z, Act H, float* bnslot,
                    bool train_bn, hipStream_t st, float* tab_out = nullptr) {
    const int C = L.n_out;
    const int64_t Mg = M * (t->ar_fn ? t->world : 1);      // rows of the global batch (equal shards per rank)
    if (L.bn) {
        float *colsum = bnslot, *m2 = bnslot + t->W, *mean = bnslot + 2 * t->W, *istd = bnslot + 3 * t->W;
        if (train_bn && rows_ok(engine_policy(t), M, L.n_in, L.n_out)) {
            // batch statistics from the GEMM epilogue: shifted sums (shift = 30 b) in double, no extra pass over Z
            // t->bn_stats is zero here: every consumer of the sums clears them (and each pass starts with one memset)
            HIPCK(linear_fwd(t, L, In, M, Z.p, Z.ld, 30.f, nullptr, st, t->bn_stats));
            RC(all_reduce(t, t->bn_stats, 2 * C, true, st));          // the shift 30 b is the same on every rank: the sums add
            HIPCK(launch_bn_finalize_shifted(t->bn_stats, t->params + L.b, 30.f, Mg, C, mean, istd, t->buffers + L.rm, t->buffers + L.rv,
                                             t->params + L.g, t->params + L.beta, tab_out, st));
            if (tab_out) return SNERF_OK;                               // the table is written; no sin pass with activation on load
        } else if (train_bn) {
            HIPCK(snerf_zero_async(bnslot, 0, 2 * t->W * sizeof(float), st));
            HIPCK(linear_fwd(t, L, In, M, Z.p, Z.ld, 30.f, colsum, st));
            RC(all_reduce(t, colsum, C, false, st));
            HIPCK(launch_bn_finalize(colsum, m2, Mg, C, mean, istd, nullptr, nullptr, 0, st));
            ColArgs ca{};
            ca.mode = 0; ca.M = M; ca.C = C; ca.ld = Z.ld; ca.Z = Z.p; ca.mu = mean; ca.out0 = m2; ca.alpha0 = 1.f;
            HIPCK(launch_colreduce(ca, st));
            RC(all_reduce(t, m2, C, false, st));
            HIPCK(launch_bn_finalize(colsum, m2, Mg, C, mean, istd, t->buffers + L.rm, t->buffers + L.rv, 1, st));
        } else {      // eval-mode statistics (running estimates)
            HIPCK(linear_fwd(t, L, In, M, Z.p, Z.ld, 30.f, nullptr, st));
            HIPCK(snerf_copy_async(mean, t->buffers + L.rm, C * sizeof(float), st));
            // istd from running var: reuse finalize stage 1 arithmetic with M = 1 via a tiny dedicated path
            HIPCK(launch_bn_finalize(nullptr, t->buffers + L.rv, 1, C, mean, istd, nullptr, nullptr, 2, st));
        }
        if (tab_out) HIPCK(launch_act_table(mean, istd, t->params + L.g, t->params + L.beta, C, tab_out, st));
        else HIPCK(launch_sin_fwd(Z.p, H.p, M, C, Z.ld, H.ld, mean, istd, t->params + L.g, t->params + L.beta, st));
    } else {
        HIPCK(linear_fwd(t, L, In, M, Z.p, Z.ld, 30.f, nullptr, st));
        // without BatchNorm the table is the constant [1/(2 pi) | 0]: written once at bind time (const_tables)
        if (!tab_out) HIPCK(launch_sin_fwd(Z.p, H.p, M, C, Z.ld, H.ld, nullptr, nullptr, nullptr, nullptr, st));
    }
    return SNERF_OK;
}

// SineLayer backward.  D holds dL/dH on entry ([M, n_out], ld = D.ld) and dL/dZ on exit (in place).
// Accumulates weight/bias (and BN affine) gradients; if dIn.p != null writes dL/dIn[:, :n_in_cols].
static int sine_bwd(snerf_trainer* t, const LayerP& L, Act D, Act Z, Act In, int64_t M, float* bnslot,
                    Act dIn, int n_in_cols, bool accumulate_in, hipStream_t st, bool pre_activated = false,
                    const ActBelow* below = nullptr, bool* fused_below = nullptr, bool batch_bn = true) {
    // pre_activated: the dgrad that produced D already applied this layer's activation backward (D = dL/dH * cos) and left the
    // column sums in t->bn_stats.  below / fused_below: the same offer for the layer that will consume dIn.
    // batch_bn: the forward normalised with batch statistics.  false (train_bn = 0, running estimates): mean and istd do not depend on
    // the batch, so dZ = gamma istd dY; d beta and d gamma keep their form, with xhat taken from the running estimates.
    const int C = L.n_out;
    if (fused_below) *fused_below = false;
    // EXPERIMENT (never on by default): the inter-layer gradient as bf16.  Rounds dL/dY (as the dgrad above would have stored it) and, behind the
    // weight-gradient kernel, dL/dZ (as it would be written back) to bf16 precision in place: the accuracy side of the idea on the real kernels.
    const bool dy_bf16 = switches().dy_bf16;
    if (dy_bf16 && pre_activated) HIPCK(launch_round_bf16(D.p, D.ld, M, C, st));
    WgradBN bn{}, *ride = nullptr;      // ride set: the BatchNorm dZ pass rides in the weight-gradient kernel
    if (L.bn) {
        float *mean = bnslot + 2 * t->W, *istd = bnslot + 3 * t->W;
        float *sdy = t->bn_bwd, *sdyx = t->bn_bwd + t->W;
        HIPCK(snerf_zero_async(t->bn_bwd, 0, 2 * t->W * sizeof(float), st));      // [2][W]: a narrower layer leaves the tails zero (the
                                                                                 // whole buffer goes through the sync-BatchNorm all-reduce)
        if (pre_activated) {
            // d beta += sum dY, d gamma += sum dY*xhat (per-rank sums), and the fp32 copies the dZ pass reads
            HIPCK(launch_act_sums_finalize(t->bn_stats, C, 1.f, sdy, sdyx, t->grads + L.beta, t->grads + L.g, st));
        } else {
            ColArgs ca{};
            ca.mode = 1; ca.M = M; ca.C = C; ca.ld = Z.ld; ca.Z = Z.p; ca.D = D.p; ca.mu = mean; ca.istd = istd;
            ca.gamma = t->params + L.g; ca.beta = t->params + L.beta; ca.out0 = sdy; ca.out1 = sdyx; ca.alpha0 = 1.f;
            ca.ldd = D.ld;
            HIPCK(launch_colreduce(ca, st));
            // d beta = sum dY, d gamma = sum dY*xhat
            HIPCK(launch_copy_cols(sdy, C, t->grads + L.beta, C, 1, C, true, st));       // parameter gradients stay per-rank sums
            HIPCK(launch_copy_cols(sdyx, C, t->grads + L.g, C, 1, C, true, st));
        }
        if (batch_bn) RC(all_reduce(t, t->bn_bwd, 2 * t->W, false, st));                 // the BatchNorm backward means are global
        // frozen statistics: the sums have gone into d beta / d gamma above.  With both at zero every dZ form below (bn_bwd2, its column-pass
        // twins, the ride in the weight-gradient kernel) computes gamma istd (dY - 0 - xhat 0) = gamma istd dY exactly; d bias = 30 sum dZ follows
        else HIPCK(snerf_zero_async(t->bn_bwd, 0, 2 * t->W * sizeof(float), st));
        const int64_t Mg = M * (t->ar_fn ? t->world : 1);
        // D holds dL/dY: the dZ sweep rides in the weight-gradient kernel (dY -> dZ in registers, written back in place) or is a pass of its own
        bn = WgradBN{Z.p, Z.ld, t->params + L.g, mean, istd, sdy, sdyx, 1.f / (float)Mg, 30.f, t->grads + L.b};
        if (pre_activated && wgrad_rows_ok(engine_policy(t), M)) ride = &bn;
        else HIPCK(launch_bn_bwd2(Z.p, D.p, M, C, Z.ld, D.ld, mean, istd, t->params + L.g, t->params + L.beta, sdy, sdyx, t->grads + L.b, 30.f, Mg, st, pre_activated));
    } else if (pre_activated) {
        HIPCK(launch_act_sums_finalize(t->bn_stats, C, 30.f, nullptr, nullptr, t->grads + L.b, nullptr, st));     // d bias = 30 * sum dZ
    } else {
        ColArgs ca{};
        ca.mode = 2; ca.M = M; ca.C = C; ca.ld = Z.ld; ca.ldd = D.ld; ca.Z = Z.p; ca.D = D.p; ca.out0 = t->grads + L.b; ca.alpha0 = 30.f;
        HIPCK(launch_colreduce(ca, st));
    }
    HIPCK(linear_wgrad(t, L, D.p, D.ld, In, M, 30.f, st, ride));
    if (ride && dy_bf16) HIPCK(launch_round_bf16(D.p, D.ld, M, C, st));
    if (dIn.p) HIPCK(linear_dgrad(t, L, D.p, D.ld, M, dIn.p, dIn.ld, n_in_cols, 30.f, accumulate_in, st, below, fused_below));
    return SNERF_OK;
}

// The colour head (3 outputs) and the density head (1) read the same input X1, and their outputs - and output gradients - sit side by side in an [N, 4]
// buffer Y: one K = 4 product on the thin route (row 3 of the weights / results at the density head's addresses; input gradient added to dX1).  false: the layers do not fit.
static bool heads_product(const snerf_trainer* t, const Act& X1, int64_t N, float* Y, Product* p) {
    const LayerP &Lc = t->layers[L_COL], &Ld = t->layers[L_SIG];
    if (Lc.n_out != 3 || Ld.n_out != 1 || Lc.n_in != Ld.n_in) return false;
    *p = product_of(t, Lc, X1, N, Y, 4, 1.f);
    p->n_out = 4; p->W3 = t->params + Ld.w; p->bias3 = t->params + Ld.b; p->dW3 = t->grads + Ld.w;
    p->dX = t->dX1.p; p->lddx = t->W2; p->n_cols = Lc.n_in; p->accumulate = true;
    return true;
}
// plain Linear (heads): Out[M, n_out] = In W^T + b
static hipError_t plain_fwd(snerf_trainer* t, const LayerP& L, Act In, int64_t M, float* Out, int64_t ldo, hipStream_t st) {
    return linear_fwd(t, L, In, M, Out, ldo, 1.f, nullptr, st, nullptr, true);
}
static int plain_bwd(snerf_trainer* t, const LayerP& L, float* dOut, int64_t ldo, Act In, int64_t M,
                     float* dIn, int64_t ld_din, bool accumulate, hipStream_t st, const ActBelow* below = nullptr, bool* fused_below = nullptr) {
    if (fused_below) *fused_below = false;
    HIPCK(linear_wgrad(t, L, dOut, ldo, In, M, 1.f, st));
    HIPCK(launch_colsum(dOut, M, L.n_out, ldo, 1.f, t->grads + L.b, st));
    if (dIn) HIPCK(linear_dgrad(t, L, dOut, ldo, M, dIn, ld_din, L.n_in, 1.f, accumulate, st, below, fused_below));
    return SNERF_OK;
}

static int forward_pass(snerf_trainer* t, snerf_trainer::Pass& P, bool solar, int64_t R, int S, const float* top, const float* bot,
                        const float* tvals, const float* sun, const float* time, bool train_bn, hipStream_t st,
                        float* adjust_col_out = nullptr) {
    const int W = t->W, W2 = t->W2, W4 = t->W4, C = t->C;
    const int64_t N = R * S;
    // the column-sum scratch starts every pass at zero (its consumers clear what they read: no memset per layer)
    HIPCK(snerf_zero_async(t->bn_stats, 0, (size_t)(4 * W + 2) * sizeof(float), st));
    HIPCK(snerf_copy_async(P.top, top, R * 3 * sizeof(float), st));
    HIPCK(snerf_copy_async(P.bot, bot, R * 3 * sizeof(float), st));
    HIPCK(snerf_copy_async(P.tvals, tvals, S * sizeof(float), st));
    auto& Ls = t->layers;
    PeArgs pa{};
    pa.n = N; pa.n_samples = S; pa.top = top; pa.bot = bot; pa.tvals = tvals; pa.pe = P.E.p; pa.pts = P.pts;
    pa.pe2 = P.In5.p + W; pa.ld2 = W + 64;                  // second copy: the PE columns of fc5's concat input
    HIPCK(launch_pe_points(pa, st));
    // Activation on load (per-point layers): store only the pre-activations Z; every consumer applies sin(BN(.)) while loading.
    // Needs the bf16x3 kernels for every consumer (K <= 512, widths multiples of 16) and enough points for them to be used.
    const bool aol = t->aol_mode == 1 && W % 16 == 0 && rows_ok(engine_policy(t), N, W + 64, 1);
    P.aol = aol;
    P.batch_bn = train_bn;
    auto view = [&](Act Z, Act H, int slot, int n) { return aol ? Act{Z.p, Z.ld, P.tab(slot, W), n} : H; };
    // fc4's output lives inside fc5's concat input [ . | PE]: its H without, its Z with activation on load
    // likewise fc9's inside fc_solar_1's concat input [ . | PE(sun)]
    P.Zc3 = aol ? Act{P.In5.p, W + 64} : P.Z[3];
    P.Zc8 = aol ? Act{P.In_s1.p, P.In_s1.ld} : P.Z[8];
    auto zof = [&](int l) { return l == 3 ? P.Zc3 : (l == 8 ? P.Zc8 : P.Z[l]); };
    for (int l = 0; l < 9; ++l) P.Hc[l] = view(zof(l), P.H[l], l, l == 8 ? W2 : W);
    for (int l = 0; l < 3; ++l) { P.Hac[l] = view(P.Za[l], P.Ha[l], 9 + l, W); P.Hsc[l] = view(P.Zs[l], P.Hs[l], 12 + l, W2); }
    P.In5c = aol ? Act{P.In5.p, W + 64, P.tab(3, W), W, true} : Act{P.In5.p, W + 64, nullptr, 0, true};      // column W+63 is the PE's zero pad
    P.In_s1c = aol ? Act{P.In_s1.p, P.In_s1.ld, P.tab(8, W), W2, true} : Act{P.In_s1.p, P.In_s1.ld, nullptr, 0, true};
    // trunk (G_NeRF.py:80-91)
    RC(sine_fwd(t, Ls[L_FC1], Act{P.E.p, 64, nullptr, 0, true}, N, P.Z[0], P.H[0], nullptr, train_bn, st, P.tab(0, W)));
    for (int l = 1; l < 9; ++l) {
        const Act In = l == 4 ? P.In5c : P.Hc[l - 1];
        RC(sine_fwd(t, Ls[L_FC1 + l], In, N, zof(l), P.H[l], P.bn + (l - 1) * 4 * W, train_bn, st, P.tab(l, W)));
    }
    const Act X1 = P.Hc[8];
    {   // colour (3) and density (1) heads: one stream over X1 for both where it applies (thin_fwd_kernel), else one product each
        Product hp;
        if (heads_product(t, X1, N, P.head.p, &hp) && route_fwd(hp, engine_policy(t, true)) == Route::Thin) {
            HIPCK(run_fwd(hp, Route::Thin, st));
        } else {
            HIPCK(plain_fwd(t, Ls[L_COL], X1, N, P.head.p, 4, st));
            HIPCK(plain_fwd(t, Ls[L_SIG], X1, N, P.head.p + 3, 4, st));
        }
    }
    // solar visibility branch (G_NeRF.py:100-108)
    HIPCK(launch_pe_small(sun, 3, 3, 4, R, P.pe_sun, 28, st));
    if (!aol) HIPCK(launch_copy_cols(X1.p, X1.ld, P.In_s1.p, P.In_s1.ld, N, W2, false, st));
    HIPCK(launch_bcast_rows(P.pe_sun, 28, P.In_s1.p, P.In_s1.ld, W2, N, S, st));
    RC(sine_fwd(t, Ls[L_S1], P.In_s1c, N, P.Zs[0], P.Hs[0], nullptr, train_bn, st, P.tab(12, W)));
    RC(sine_fwd(t, Ls[L_S2], P.Hsc[0], N, P.Zs[1], P.Hs[1], nullptr, train_bn, st, P.tab(13, W)));
    RC(sine_fwd(t, Ls[L_S3], P.Hsc[1], N, P.Zs[2], P.Hs[2], nullptr, train_bn, st, P.tab(14, W)));
    HIPCK(plain_fwd(t, Ls[L_S4], P.Hsc[2], N, P.sv_raw.p, 1, st));
    // sky colour head (G_NeRF.py:110-111), per ray
    RC(sine_fwd(t, Ls[L_K1], Act{P.pe_sun, 28}, R, Act{P.Zk1, W4}, Act{P.Hk1, W4}, nullptr, train_bn, st));
    HIPCK(plain_fwd(t, Ls[L_K2], Act{P.Hk1, W4}, R, P.sky_raw, 3, st));
    HIPCK(launch_sigmoid(P.sky_raw, P.sky, R * 3, st));
    PointOutArgs po{};
    po.n = N; po.n_samples = S; po.C = C; po.head = P.head.p; po.sv_raw = P.sv_raw.p; po.rho = P.rho; po.sv = P.sv;
    if (!solar) {
        // seasonal colour-adjust branch (T_NeRF_net_v2.py:83-88) and time -> class softmax (:77-78, per ray)
        RC(sine_fwd(t, Ls[L_A1], X1, N, P.Za[0], P.Ha[0], nullptr, train_bn, st, P.tab(9, W)));
        RC(sine_fwd(t, Ls[L_A2], P.Hac[0], N, P.Za[1], P.Ha[1], nullptr, train_bn, st, P.tab(10, W)));
        RC(sine_fwd(t, Ls[L_A3], P.Hac[1], N, P.Za[2], P.Ha[2], nullptr, train_bn, st, P.tab(11, W)));
        HIPCK(plain_fwd(t, Ls[L_AC], P.Hac[2], N, P.adj.p, 3 * C, st));
        HIPCK(launch_pe_small(time, 4, 2, 2, R, P.pe_time, 12, st));
        RC(sine_fwd(t, Ls[L_T1], Act{P.pe_time, 12}, R, Act{P.Zt1, W}, Act{P.Ht1, W}, nullptr, train_bn, st));
        RC(sine_fwd(t, Ls[L_T2], Act{P.Ht1, W}, R, Act{P.Zt2, W}, Act{P.Ht2, W}, nullptr, train_bn, st));
        HIPCK(plain_fwd(t, Ls[L_CL], Act{P.Ht2, W}, R, P.logits, C, st));
        HIPCK(launch_softmax(P.logits, P.cls, R, C, st));
        po.adj = P.adj.p; po.cls = P.cls; po.col = P.col; po.adjust_col = adjust_col_out;
    }
    HIPCK(launch_point_out(po, false, st));
    return SNERF_OK;
}

extern "C" {

static std::mutex g_live_mu;
static std::set<const snerf_trainer*> g_live;          // trainers created and not yet destroyed

snerf_trainer* snerf_trainer_create(int layer_width, int n_classes) {
    if (layer_width < 16 || layer_width % 4 != 0 || n_classes < 1 || n_classes > 5) {
        snerf_set_error(SNERF_E_INVALID, "snerf_trainer_create: width must be a multiple of 4 (>=16), classes in [1,5]");
        return nullptr;
    }
    snerf_trainer* t = new snerf_trainer();
    t->W = layer_width; t->C = n_classes; t->W2 = layer_width / 2; t->W4 = layer_width / 4;
    if (const char* e = getenv("SNERF_TRAIN_GEMM")) t->gemm_mode = std::strcmp(e, "fp32") == 0 ? 0 : 1;
    if (const char* e = getenv("SNERF_TRAIN_AOL")) t->aol_mode = std::strcmp(e, "0") == 0 ? 0 : 1;
    build_layers(t);
    {
        std::lock_guard<std::mutex> lock(g_live_mu);
        g_live.insert(t);
    }
    return t;
}
void snerf_trainer_destroy(snerf_trainer* t) {
    {
        std::lock_guard<std::mutex> lock(g_live_mu);
        g_live.erase(t);
    }
    delete t;
}
// Class count of a LIVE trainer, -1 for a pointer that is not one (never created here, or destroyed): what a caller that holds the handle as
// a plain integer (the PyTorch custom ops, csrc/ops.cpp) checks before it dereferences it or sizes an output by a class count.
int snerf_trainer_classes(const snerf_trainer* t) {
    std::lock_guard<std::mutex> lock(g_live_mu);
    return g_live.count(t) ? t->C : -1;
}
int snerf_trainer_bound_sizes(const snerf_trainer* t, int64_t* n_rays, int64_t* n_solar_rays, int* n_samples) {
    if (!t || !t->ws) return snerf_set_error(SNERF_E_STATE, "trainer not bound (call snerf_trainer_bind)");
    if (n_rays) *n_rays = t->R;
    if (n_solar_rays) *n_solar_rays = t->Rs;
    if (n_samples) *n_samples = t->S;
    return SNERF_OK;
}
int64_t snerf_trainer_param_floats(const snerf_trainer* t) { return t ? t->n_params : 0; }
int64_t snerf_trainer_buffer_floats(const snerf_trainer* t) { return t ? t->n_buffers : 0; }
int snerf_trainer_tensor_count(const snerf_trainer* t) {
    if (!t) return 0;
    int n = 0;
    for (const LayerP& l : t->layers) n += 2 + (l.bn ? 4 : 0);
    return n;
}
int snerf_trainer_tensor_info(const snerf_trainer* t, int index, char* key, int key_cap, int* is_buffer, int64_t* offset,
                              int64_t* numel, int* rows, int* cols) {
    if (!t || !key) return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_tensor_info: bad argument");
    int i = 0;
    for (const LayerP& l : t->layers) {
        const std::string lin = l.sine ? l.name + ".linear" : l.name;
        struct Ent { std::string k; int buf; int64_t off, n; int r, c; };
        std::vector<Ent> ents = {{lin + ".weight", 0, l.w, (int64_t)l.n_out * l.n_in, l.n_out, l.n_in}, {lin + ".bias", 0, l.b, l.n_out, l.n_out, 1}};
        if (l.bn) {
            ents.push_back({l.name + ".norm.weight", 0, l.g, l.n_out, l.n_out, 1});
            ents.push_back({l.name + ".norm.bias", 0, l.beta, l.n_out, l.n_out, 1});
            ents.push_back({l.name + ".norm.running_mean", 1, l.rm, l.n_out, l.n_out, 1});
            ents.push_back({l.name + ".norm.running_var", 1, l.rv, l.n_out, l.n_out, 1});
        }
        for (const Ent& e : ents) {
            if (i == index) {
                std::strncpy(key, e.k.c_str(), key_cap - 1);
                key[key_cap - 1] = 0;
                if (is_buffer) *is_buffer = e.buf;
                if (offset) *offset = e.off;
                if (numel) *numel = e.n;
                if (rows) *rows = e.r;
                if (cols) *cols = e.c;
                return SNERF_OK;
            }
            ++i;
        }
    }
    return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_tensor_info: index out of range");
}

size_t snerf_trainer_workspace_bytes(snerf_trainer* t, int64_t n_rays, int64_t n_solar_rays, int n_samples) {
    if (!t) return 0;
    snerf_trainer tmp = *t;
    return carve(&tmp, nullptr, n_rays, n_solar_rays, n_samples);
}

int snerf_trainer_bind(snerf_trainer* t, float* d_params, float* d_grads, float* d_adam_m, float* d_adam_v, float* d_buffers,
                       void* d_workspace, size_t workspace_bytes, int64_t n_rays, int64_t n_solar_rays, int n_samples) {
    if (!t || !d_params || !d_grads || !d_buffers || !d_workspace || n_rays < 0 || n_solar_rays < 0 || n_samples < 1)
        return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_bind: bad argument");
    const size_t need = snerf_trainer_workspace_bytes(t, n_rays, n_solar_rays, n_samples);
    if (workspace_bytes < need) return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_bind: workspace too small");
    t->params = d_params; t->grads = d_grads; t->adam_m = d_adam_m; t->adam_v = d_adam_v; t->buffers = d_buffers;
    t->ws = (char*)d_workspace; t->ws_bytes = workspace_bytes;
    t->R = n_rays; t->Rs = n_solar_rays; t->S = n_samples;
    carve(t, t->ws, n_rays, n_solar_rays, n_samples);
    for (snerf_trainer::Pass* P : {&t->img, &t->sol}) {
        // the zero pad columns of the solar branch's concat input
        if (P->N > 0) HIPCK(hipMemset(P->In_s1.p, 0, (size_t)P->N * P->In_s1.ld * sizeof(float)));
        // activation-on-load tables of the layers without BatchNorm (fc1, adjust 1-3, solar 1-3) are constants: [1/(2 pi) | 0]
        const int slots[7] = {0, 9, 10, 11, 12, 13, 14};
        for (int sl : slots) HIPCK(launch_act_table(nullptr, nullptr, nullptr, nullptr, sl >= 12 ? t->W2 : t->W, P->tabs + (int64_t)sl * 2 * t->W, nullptr));
    }
    HIPCK(hipMemset(t->bn_stats, 0, (size_t)(4 * t->W + 2) * sizeof(float)));
    HIPCK(hipDeviceSynchronize());
    return SNERF_OK;
}

static int check_bound(const snerf_trainer* t, int64_t R, int S, bool solar) {
    if (!t || !t->ws) return snerf_set_error(SNERF_E_STATE, "trainer not bound (call snerf_trainer_bind)");
    if (S != t->S || R != (solar ? t->Rs : t->R)) return snerf_set_error(SNERF_E_INVALID, "ray/sample counts differ from the bound sizes");
    return SNERF_OK;
}

int snerf_trainer_forward_image(snerf_trainer* t, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot,
                                const float* d_tvals, const float* d_sun, const float* d_time, int train_bn, int flags,
                                const snerf_composite_out* out, float* d_sky, float* d_classes, const snerf_field_out* per_sample,
                                void* stream) {
    RC(check_bound(t, n_rays, n_samples, false));
    if (!d_top || !d_bot || !d_tvals || !d_sun || !d_time || !out) return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_forward_image: bad argument");
    // the compositing backward differentiates the plain segment length: with bit 1 the gradients would be those of another function
    if (flags & 2) return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_forward_image: flags bit 1 (zero segment length outside the cube) has no backward");
    CtxGuard ctx(t);
    t->img_flags = flags;
    hipStream_t st = (hipStream_t)stream;
    RC(forward_pass(t, t->img, false, n_rays, n_samples, d_top, d_bot, d_tvals, d_sun, d_time, train_bn != 0, st,
                    per_sample ? per_sample->d_adjust_col : nullptr));
    snerf_trainer::Pass& P = t->img;
    RC(snerf_composite_rays(n_rays, n_samples, d_top, d_bot, d_tvals, P.rho, P.col, P.sv, P.sky, flags, nullptr, 1.f, out, stream));
    const int64_t N = n_rays * n_samples;
    if (d_sky) HIPCK(snerf_copy_async(d_sky, P.sky, n_rays * 3 * sizeof(float), st));
    if (d_classes) HIPCK(snerf_copy_async(d_classes, P.cls, n_rays * t->C * sizeof(float), st));
    if (per_sample) {
        if (per_sample->d_rho) HIPCK(snerf_copy_async(per_sample->d_rho, P.rho, N * 4, st));
        if (per_sample->d_solar_vis) HIPCK(snerf_copy_async(per_sample->d_solar_vis, P.sv, N * 4, st));
        if (per_sample->d_col) HIPCK(snerf_copy_async(per_sample->d_col, P.col, N * 12, st));
        if (per_sample->d_points) HIPCK(snerf_copy_async(per_sample->d_points, P.pts, N * 12, st));
        if (per_sample->d_col_raw) HIPCK(launch_copy_cols(P.head.p, 4, per_sample->d_col_raw, 3, N, 3, false, st));
        if (per_sample->d_adjust) HIPCK(snerf_copy_async(per_sample->d_adjust, P.adj.p, N * 3 * t->C * 4, st));
    }
    return SNERF_OK;
}

// Backward of the image pass through the network, from the per-sample gradients already sitting in the workspace:
// t->d_rho [N], t->d_col [N,3], t->d_sky [R,3] and - when `classic` (the solar visibility carries gradient) - dL/dSolar_Vis
// in t->d_sv_raw [N].  d_g_classes (optional, [R,C]) is added to the class-probability gradient.
static int network_backward_image(snerf_trainer* t, bool classic, const float* d_g_classes, hipStream_t st);

static int backward_image(snerf_trainer* t, const float* d_g_rgb, const float* d_g_albedo, const float* d_g_sky,
                          const float* d_g_pe, const float* d_rho_prior, float trust, const float* d_trust, const float* d_g_rgb_merged,
                          const float* d_g_albedo_merged, void* stream) {
    if (!t || !t->ws) return snerf_set_error(SNERF_E_STATE, "trainer not bound");
    CtxGuard ctx(t);
    hipStream_t st = (hipStream_t)stream;
    snerf_trainer::Pass& P = t->img;
    const int S = t->S;
    const int64_t R = P.R;
    CompBwdArgs cb{};
    cb.n_rays = R; cb.n_samples = S; cb.top = P.top; cb.bot = P.bot; cb.rho = P.rho; cb.col = P.col; cb.sv = P.sv; cb.sky = P.sky;
    cb.g_rgb = d_g_rgb; cb.g_albedo = d_g_albedo; cb.g_pe = d_g_pe; cb.d_rho = t->d_rho; cb.d_col = t->d_col; cb.d_sky = t->d_sky;
    cb.rho_prior = d_rho_prior; cb.trust = trust; cb.trust_dev = d_trust; cb.g_rgb_m = d_g_rgb_merged; cb.g_albedo_m = d_g_albedo_merged;
    const bool classic = (t->img_flags & 1) != 0;
    cb.classic = classic ? 1 : 0; cb.d_sv = t->d_sv_raw;       // dL/dSolar_Vis, turned into dL/d(raw) in place below
    HIPCK(launch_composite_bwd(cb, st));
    if (d_g_sky) HIPCK(launch_copy_cols(d_g_sky, 3, t->d_sky, 3, R, 3, true, st));
    return network_backward_image(t, classic, nullptr, st);
}

int snerf_trainer_backward_image(snerf_trainer* t, const float* d_g_rgb, const float* d_g_albedo, const float* d_g_sky,
                                 const float* d_g_pe, const float* d_rho_prior, float trust, const float* d_g_rgb_merged,
                                 const float* d_g_albedo_merged, void* stream) {
    return backward_image(t, d_g_rgb, d_g_albedo, d_g_sky, d_g_pe, d_rho_prior, trust, nullptr, d_g_rgb_merged, d_g_albedo_merged, stream);
}

int snerf_trainer_backward_image_dt(snerf_trainer* t, const float* d_g_rgb, const float* d_g_albedo, const float* d_g_sky,
                                    const float* d_g_pe, const float* d_rho_prior, const float* d_trust, const float* d_g_rgb_merged,
                                    const float* d_g_albedo_merged, void* stream) {
    if (d_rho_prior && !d_trust) return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_backward_image_dt: d_trust is NULL");
    return backward_image(t, d_g_rgb, d_g_albedo, d_g_sky, d_g_pe, d_rho_prior, 1.f, d_trust, d_g_rgb_merged, d_g_albedo_merged, stream);
}

// Seam B1 in train mode (T_NeRF.forward called on points with autograd, T_NeRF_net_v2.py:75-105): backward from gradients with
// respect to the per-sample network outputs instead of the composited colours.  Any of the pointers may be NULL (= zero).
int snerf_trainer_backward_points(snerf_trainer* t, const float* d_g_rho, const float* d_g_col, const float* d_g_solar_vis,
                                  const float* d_g_sky, const float* d_g_classes, void* stream) {
    if (!t || !t->ws) return snerf_set_error(SNERF_E_STATE, "trainer not bound");
    CtxGuard ctx(t);
    hipStream_t st = (hipStream_t)stream;
    snerf_trainer::Pass& P = t->img;
    const int64_t R = P.R, N = P.N;
    auto put = [&](float* dst, const float* src, int64_t n) -> hipError_t {
        return src ? snerf_copy_async(dst, src, n * sizeof(float), st) : snerf_zero_async(dst, 0, n * sizeof(float), st);
    };
    HIPCK(put(t->d_rho, d_g_rho, N));
    HIPCK(put(t->d_col, d_g_col, N * 3));
    HIPCK(put(t->d_sky, d_g_sky, R * 3));
    if (d_g_solar_vis) HIPCK(put(t->d_sv_raw, d_g_solar_vis, N));
    return network_backward_image(t, d_g_solar_vis != nullptr, d_g_classes, st);
}

// Backward of the colour and density heads: where the K = 4 form applies (heads_product; SNERF_FUSED_HEADS, bf16x3 mode, enough rows), ONE stream over X1 for
// both weight gradients and ONE read-modify-write of dX1 for both input gradients instead of two of each.  Which form runs is decided before the first
// launch: both accumulate into the same gradients, so a failed launch is an error, never a reason to run the other form.
static int heads_bwd(snerf_trainer* t, const Act& X1, int64_t N, const ActBelow* below, bool* fused_below, hipStream_t st) {
    const LayerP &Lc = t->layers[L_COL], &Ld = t->layers[L_SIG];
    const Policy pol = engine_policy(t, true);
    Product p;
    const bool fits = heads_product(t, X1, N, t->d_head, &p);
    if (fits) p.below = epilogue_of(t, below, p.n_cols);
    if (!fits || route_wgrad(p, pol) != Route::Thin || route_dgrad(p, pol) != Route::Thin) {
        RC(plain_bwd(t, Lc, t->d_head, 4, X1, N, t->dX1.p, t->W2, true, st));
        return plain_bwd(t, Ld, t->d_head + 3, 4, X1, N, t->dX1.p, t->W2, true, st, below, fused_below);
    }
    HIPCK(run_wgrad(p, Route::Thin, st));
    HIPCK(launch_colsum(t->d_head, N, 3, 4, 1.f, t->grads + Lc.b, st));
    HIPCK(launch_colsum(t->d_head + 3, N, 1, 4, 1.f, t->grads + Ld.b, st));
    HIPCK(run_dgrad(p, Route::Thin, st));
    if (fused_below) *fused_below = p.below.z != nullptr;
    return SNERF_OK;
}

static int network_backward_image(snerf_trainer* t, bool classic, const float* d_g_classes, hipStream_t st) {
    snerf_trainer::Pass& P = t->img;
    const int W = t->W, W2 = t->W2, W4 = t->W4, C = t->C, S = t->S;
    const int64_t R = P.R, N = P.N;
    auto& Ls = t->layers;
    if (d_g_classes) HIPCK(snerf_copy_async(t->d_cls, d_g_classes, R * C * sizeof(float), st));
    else HIPCK(snerf_zero_async(t->d_cls, 0, R * C * sizeof(float), st));
    HIPCK(snerf_zero_async(t->bn_stats, 0, (size_t)(4 * W + 2) * sizeof(float), st));      // column-sum scratch: zero at the start of the pass
    PointOutArgs po{};
    po.n = N; po.n_samples = S; po.C = C; po.head = P.head.p; po.adj = P.adj.p; po.cls = P.cls; po.col = P.col; po.sv = P.sv;
    po.d_rho = t->d_rho; po.d_col = t->d_col; po.d_head = t->d_head; po.d_adj = t->d_adj; po.d_cls = t->d_cls;
    if (classic) { po.d_sv = t->d_sv_raw; po.d_sv_raw = t->d_sv_raw; }
    HIPCK(launch_point_out(po, true, st));
    const Act X1 = P.Hc[8];
    // adjust branch
    // `pre`: did the dgrad that produced this layer's output gradient already apply its activation backward (ActBelow)?
    bool pre = false;
    {
        const ActBelow b3{&Ls[L_A3], P.Za[2], P.tab(11, W), nullptr}, b2{&Ls[L_A2], P.Za[1], P.tab(10, W), nullptr}, b1{&Ls[L_A1], P.Za[0], P.tab(9, W), nullptr};
        RC(plain_bwd(t, Ls[L_AC], t->d_adj, 3 * C, P.Hac[2], N, t->dA.p, W, false, st, &b3, &pre));
        RC(sine_bwd(t, Ls[L_A3], Act{t->dA.p, W}, P.Za[2], P.Hac[1], N, nullptr, Act{t->dB.p, W}, W, false, st, pre, &b2, &pre));
        RC(sine_bwd(t, Ls[L_A2], Act{t->dB.p, W}, P.Za[1], P.Hac[0], N, nullptr, Act{t->dA.p, W}, W, false, st, pre, &b1, &pre));
        RC(sine_bwd(t, Ls[L_A1], Act{t->dA.p, W}, P.Za[0], X1, N, nullptr, Act{t->dX1.p, W2}, W2, false, st, pre));
    }
    // sigma / colour heads
    // dL/dX1 is summed from the adjust branch, the two heads and (classic solar) the solar branch: the LAST of these dgrads
    // also applies fc9's activation backward in its epilogue
    const ActBelow b9{&Ls[L_FC9], P.Zc8, P.tab(8, W), P.bn + 7 * 4 * W};
    bool pre9 = false;
    RC(heads_bwd(t, X1, N, classic ? nullptr : &b9, classic ? nullptr : &pre9, st));
    if (classic) {      // the solar-visibility branch carries gradient from the image (G_NeRF.py:100-108), on into X1
        const ActBelow s3{&Ls[L_S3], P.Zs[2], P.tab(14, W), nullptr}, s2{&Ls[L_S2], P.Zs[1], P.tab(13, W), nullptr}, s1{&Ls[L_S1], P.Zs[0], P.tab(12, W), nullptr};
        RC(plain_bwd(t, Ls[L_S4], t->d_sv_raw, 1, P.Hsc[2], N, t->dA.p, W2, false, st, &s3, &pre));
        RC(sine_bwd(t, Ls[L_S3], Act{t->dA.p, W2}, P.Zs[2], P.Hsc[1], N, nullptr, Act{t->dB.p, W2}, W2, false, st, pre, &s2, &pre));
        RC(sine_bwd(t, Ls[L_S2], Act{t->dB.p, W2}, P.Zs[1], P.Hsc[0], N, nullptr, Act{t->dA.p, W2}, W2, false, st, pre, &s1, &pre));
        RC(sine_bwd(t, Ls[L_S1], Act{t->dA.p, W2}, P.Zs[0], P.In_s1c, N, nullptr, Act{t->dX1.p, W2}, W2, true, st, pre, &b9, &pre9));
    }
    // trunk
    float* cur = t->dA.p;
    float* nxt = t->dB.p;
    auto below_of = [&](int l) {        // trunk layer l (fc{l+1}) as the consumer of a dgrad's output
        return ActBelow{&Ls[L_FC1 + l], l == 3 ? P.Zc3 : (l == 8 ? P.Zc8 : P.Z[l]), P.tab(l, W), l >= 1 ? P.bn + (l - 1) * 4 * W : nullptr};
    };
    {
        const ActBelow b = below_of(7);
        RC(sine_bwd(t, Ls[L_FC9], Act{t->dX1.p, W2}, P.Zc8, P.Hc[7], N, P.bn + 7 * 4 * W, Act{cur, W}, W, false, st, pre9, &b, &pre, P.batch_bn));
    }
    for (int l = 7; l >= 1; --l) {
        const Act In = l == 4 ? P.In5c : P.Hc[l - 1];
        const ActBelow b = below_of(l - 1);
        RC(sine_bwd(t, Ls[L_FC1 + l], Act{cur, W}, l == 3 ? P.Zc3 : P.Z[l], In, N, P.bn + (l - 1) * 4 * W, Act{nxt, W}, W, false, st, pre, &b, &pre, P.batch_bn));
        float* tmp = cur; cur = nxt; nxt = tmp;
    }
    RC(sine_bwd(t, Ls[L_FC1], Act{cur, W}, P.Z[0], Act{P.E.p, 64}, N, nullptr, Act{nullptr, 0}, 0, false, st, pre));
    // time -> class branch (per ray)
    HIPCK(launch_softmax_bwd(P.cls, t->d_cls, t->rayA, R, C, st));
    RC(plain_bwd(t, Ls[L_CL], t->rayA, C, Act{P.Ht2, W}, R, t->rayB, W, false, st));
    RC(sine_bwd(t, Ls[L_T2], Act{t->rayB, W}, Act{P.Zt2, W}, Act{P.Ht1, W}, R, nullptr, Act{t->rayA, W}, W, false, st));
    RC(sine_bwd(t, Ls[L_T1], Act{t->rayA, W}, Act{P.Zt1, W}, Act{P.pe_time, 12}, R, nullptr, Act{nullptr, 0}, 0, false, st));
    // sky colour head (per ray)
    HIPCK(launch_sigmoid_bwd(P.sky, t->d_sky, t->rayB, R * 3, st));
    RC(plain_bwd(t, Ls[L_K2], t->rayB, 3, Act{P.Hk1, W4}, R, t->rayA, W4, false, st));
    RC(sine_bwd(t, Ls[L_K1], Act{t->rayA, W4}, Act{P.Zk1, W4}, Act{P.pe_sun, 28}, R, nullptr, Act{nullptr, 0}, 0, false, st));
    return SNERF_OK;
}

int snerf_trainer_forward_solar(snerf_trainer* t, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot,
                                const float* d_tvals, const float* d_sun, int train_bn, float* d_solar_vis, float* d_pv,
                                float* d_pe, float* d_sky_raw, float* d_rho, float* d_points, float* d_delta, void* stream) {
    RC(check_bound(t, n_rays, n_samples, true));
    if (!d_top || !d_bot || !d_tvals || !d_sun) return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_forward_solar: bad argument");
    CtxGuard ctx(t);
    hipStream_t st = (hipStream_t)stream;
    snerf_trainer::Pass& P = t->sol;
    RC(forward_pass(t, P, true, n_rays, n_samples, d_top, d_bot, d_tvals, d_sun, nullptr, train_bn != 0, st));
    snerf_composite_out co{};
    co.d_pv = d_pv; co.d_pe = d_pe; co.d_delta = d_delta;
    // col is not produced by the sun-ray pass: composite only needs rho (col/sv operands are dummies of the right size)
    RC(snerf_composite_rays(n_rays, n_samples, d_top, d_bot, d_tvals, P.rho, t->d_col, P.sv, P.sky, 0, nullptr, 1.f, &co, stream));
    const int64_t N = n_rays * n_samples;
    if (d_solar_vis) HIPCK(snerf_copy_async(d_solar_vis, P.sv, N * 4, st));
    if (d_sky_raw) HIPCK(snerf_copy_async(d_sky_raw, P.sky_raw, n_rays * 12, st));
    if (d_rho) HIPCK(snerf_copy_async(d_rho, P.rho, N * 4, st));
    if (d_points) HIPCK(snerf_copy_async(d_points, P.pts, N * 12, st));
    return SNERF_OK;
}

int snerf_trainer_backward_solar(snerf_trainer* t, const float* d_g_solar_vis, void* stream) {
    if (!t || !t->ws || !d_g_solar_vis) return snerf_set_error(SNERF_E_STATE, "trainer not bound / NULL gradient");
    CtxGuard ctx(t);
    hipStream_t st = (hipStream_t)stream;
    snerf_trainer::Pass& P = t->sol;
    const int W2 = t->W2;
    const int64_t N = P.N;
    auto& Ls = t->layers;
    HIPCK(snerf_zero_async(t->bn_stats, 0, (size_t)(4 * t->W + 2) * sizeof(float), st));
    PointOutArgs po{};
    po.n = N; po.n_samples = t->S; po.C = t->C; po.head = P.head.p; po.sv = P.sv; po.d_sv = d_g_solar_vis; po.d_sv_raw = t->d_sv_raw;
    HIPCK(launch_point_out(po, true, st));
    const ActBelow s3{&Ls[L_S3], P.Zs[2], P.tab(14, t->W), nullptr}, s2{&Ls[L_S2], P.Zs[1], P.tab(13, t->W), nullptr}, s1{&Ls[L_S1], P.Zs[0], P.tab(12, t->W), nullptr};
    bool pre = false;
    RC(plain_bwd(t, Ls[L_S4], t->d_sv_raw, 1, P.Hsc[2], N, t->dA.p, W2, false, st, &s3, &pre));
    RC(sine_bwd(t, Ls[L_S3], Act{t->dA.p, W2}, P.Zs[2], P.Hsc[1], N, nullptr, Act{t->dB.p, W2}, W2, false, st, pre, &s2, &pre));
    RC(sine_bwd(t, Ls[L_S2], Act{t->dB.p, W2}, P.Zs[1], P.Hsc[0], N, nullptr, Act{t->dA.p, W2}, W2, false, st, pre, &s1, &pre));
    RC(sine_bwd(t, Ls[L_S1], Act{t->dA.p, W2}, P.Zs[0], P.In_s1c, N, nullptr, Act{nullptr, 0}, 0, false, st, pre));
    return SNERF_OK;
}

// Introspection for tests: copy an internal buffer of the last image-pass backward to the host (synchronous).
int snerf_trainer_debug_read(snerf_trainer* t, const char* name, float* host_out, int64_t n_floats) {
    if (!t || !t->ws || !name || !host_out) return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_debug_read: bad argument");
    const std::string k = name;
    const float* src = k == "d_rho" ? t->d_rho : k == "d_col" ? t->d_col : k == "d_head" ? t->d_head : k == "d_adj" ? t->d_adj
                     : k == "d_sky" ? t->d_sky : k == "d_cls" ? t->d_cls : k == "rho" ? t->img.rho : k == "col" ? t->img.col
                     : k == "sv" ? t->img.sv : k == "sky" ? t->img.sky : k == "head" ? t->img.head.p : k == "d_sv_raw" ? t->d_sv_raw : nullptr;
    if (!src) return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_debug_read: unknown buffer " + k);
    HIPCK(hipDeviceSynchronize());
    HIPCK(hipMemcpy(host_out, src, n_floats * sizeof(float), hipMemcpyDeviceToHost));
    return SNERF_OK;
}

// Introspection for tests: one launcher of train.h on the caller's buffers (include/season_nerf_hip.h lists the operations and their arguments).
// Everything a launcher takes on trust is checked here first; the return value is the launcher's own *_choice where it has one.
int snerf_train_kernel_debug(const char* op, const int64_t* s, int n_sizes, const float* f, int n_scalars, void* const* p, int n_ptrs, void* stream) {
    struct OpDesc { const char* name; int ns, nf, np; };
    static const OpDesc ops[] = {
        {"pe_points", 3, 0, 7}, {"pe_small", 5, 0, 2}, {"colreduce", 5, 1, 8}, {"bn_bwd2", 6, 1, 9}, {"bn_finalize", 3, 0, 6},
        {"bn_finalize_shifted", 2, 1, 9}, {"act_sums_finalize", 1, 1, 5}, {"act_table", 1, 0, 5}, {"sin_fwd", 4, 0, 6},
        {"thin_dgrad", 8, 1, 9}, {"point_out_fwd", 3, 0, 15}, {"point_out_bwd", 3, 0, 15}, {"softmax", 2, 0, 2}, {"softmax_bwd", 2, 0, 3},
        {"sigmoid", 1, 0, 2}, {"sigmoid_bwd", 1, 0, 3}, {"colsum", 3, 1, 2}, {"copy_cols", 5, 0, 2}, {"bcast_rows", 5, 0, 2},
        {"reduce_rows", 5, 0, 2}, {"fill_zero", 1, 0, 1}, {"copy_f32", 1, 0, 2}, {"fill_zero_bytes", 1, 0, 1}, {"copy_bytes", 1, 0, 2},
        {"colpass_rows_per_block", 2, 0, 0}, {"thin_dgrad_rows_per_block", 2, 0, 0}, {"wgrad", 10, 2, 11}, {"thin_wgrad", 7, 1, 5}, {"thin_fwd", 7, 1, 7}};
    if (!op) return snerf_set_error(SNERF_E_INVALID, "snerf_train_kernel_debug: NULL operation name");
    const std::string k = op;
    const OpDesc* d = nullptr;
    for (const OpDesc& o : ops)
        if (k == o.name) d = &o;
    if (!d) return snerf_set_error(SNERF_E_INVALID, "snerf_train_kernel_debug: unknown operation " + k);
    const auto bad = [&](const char* what) { return snerf_set_error(SNERF_E_INVALID, "snerf_train_kernel_debug: " + k + ": " + what); };
    if (n_sizes != d->ns || n_scalars != d->nf || n_ptrs != d->np) return bad("wrong number of sizes, scalars or pointers");
    if ((d->ns && !s) || (d->nf && !f) || (d->np && !p)) return bad("NULL argument array");
    for (int i = 0; i < d->ns; ++i)
        if (s[i] < 0 || s[i] > ((int64_t)1 << 40)) return bad("a size is negative or too large");
    for (int i = 0; i < d->np; ++i)
        if ((uintptr_t)p[i] % 4 != 0 && k != "fill_zero_bytes" && k != "copy_bytes") return bad("a float pointer is not 4-byte aligned");
    const auto F = [&](int i) { return (float*)p[i]; };
    const auto fits_int = [&](int64_t v) { return v <= 0x7fffffff; };
    hipStream_t st = (hipStream_t)stream;
    int kernel = -1;
    hipError_t e = hipSuccess;
    if (k == "colpass_rows_per_block" || k == "thin_dgrad_rows_per_block") {
        if (s[1] < 4 || s[1] % 4 || s[1] > 1024) return bad("the column count must be a multiple of 4 in 4..1024");
        return k[0] == 'c' ? colpass_rows_per_block(s[0], (int)s[1]) : thin_dgrad_rows_per_block(s[0], (int)s[1]);
    } else if (k == "pe_points") {                  // sizes n, n_samples, ld2; pointers points, top, bot, tvals, pe, pts, pe2
        PeArgs a{};
        a.n = s[0]; a.n_samples = (int)s[1]; a.ld2 = s[2];
        a.points = F(0); a.top = F(1); a.bot = F(2); a.tvals = F(3); a.pe = F(4); a.pts = F(5); a.pe2 = F(6);
        if (!a.pe) return bad("pe is NULL");
        if (!a.points && (!a.top || !a.bot || !a.tvals || s[1] < 1 || !fits_int(s[1]) || a.n % s[1] != 0)) return bad("the rays form needs top, bot, tvals and n a multiple of n_samples >= 1");
        if (a.pe2 && a.ld2 < 64) return bad("ld2 < 64");
        kernel = TK_PE_POINTS;
        e = launch_pe_points(a, st);
    } else if (k == "pe_small") {            // sizes rows, in_stride, n_dims, n_freq, out_stride; pointers in, out
        if (!p[0] || !p[1]) return bad("NULL pointer");
        if (s[2] < 1 || s[2] > 16 || s[3] > 30 || s[1] < s[2] || !fits_int(s[1]) || !fits_int(s[4]) || s[4] < s[2] * (2 * s[3] + 1)) return bad("bad dimensions, frequencies or strides");
        kernel = TK_PE_SMALL;
        e = launch_pe_small(F(0), (int)s[1], (int)s[2], (int)s[3], s[0], F(1), (int)s[4], st);
    } else if (k == "colreduce") {           // sizes mode, M, C, ld, ldd; scalar alpha0; pointers Z, D, mu, istd, gamma, beta, out0, out1
        ColArgs a{};
        a.mode = (int)s[0]; a.M = s[1]; a.C = (int)s[2]; a.ld = s[3]; a.ldd = s[4]; a.alpha0 = f[0];
        a.Z = F(0); a.D = F(1); a.mu = F(2); a.istd = F(3); a.gamma = F(4); a.beta = F(5); a.out0 = F(6); a.out1 = F(7);
        if (s[0] > 2) return bad("mode must be 0, 1 or 2");
        if (s[2] < 1 || !fits_int(s[2]) || a.ld < a.C || (a.ldd && a.ldd < a.C)) return bad("C < 1 or a leading dimension below C");
        if (!a.Z || !a.out0 || (a.mode != 0 && !a.D)) return bad("Z, out0 or D is NULL");
        if (a.mode == 1 && (!a.mu || !a.istd || !a.gamma || !a.beta || !a.out1)) return bad("mode 1 needs mu, istd, gamma, beta and out1");
        kernel = colreduce_choice(a);
        e = launch_colreduce(a, st);
    } else if (k == "bn_bwd2") {             // sizes M, C, ld, ldd, M_global, d_is_dy; scalar alpha; pointers Z, D, mu, istd, gamma, beta, sdy, sdyx, dbias
        if (s[1] < 1 || !fits_int(s[1]) || s[2] < s[1] || (s[3] && s[3] < s[1])) return bad("C < 1 or a leading dimension below C");
        if (s[4] < s[0] || s[4] < 1) return bad("M_global must be at least M and 1");
        if (s[5] > 1) return bad("d_is_dy must be 0 or 1");
        for (int i = 0; i < 8; ++i)
            if (!p[i]) return bad("NULL pointer (only dbias is optional)");
        kernel = bn_bwd2_choice(F(0), F(1), (int)s[1], s[2], s[3], s[5] != 0);
        e = launch_bn_bwd2(F(0), F(1), s[0], (int)s[1], s[2], s[3], F(2), F(3), F(4), F(5), F(6), F(7), F(8), f[0], s[4], st, s[5] != 0);
    } else if (k == "bn_finalize") {         // sizes M, C, stage; pointers colsum, m2, mean, istd, running_mean, running_var
        if (s[1] < 1 || !fits_int(s[1]) || s[2] > 2) return bad("C < 1 or stage outside 0..2");
        if (s[2] != 2 && s[0] < 1) return bad("M < 1");
        if (s[2] == 0 ? (!p[0] || !p[2]) : (!p[1] || !p[3])) return bad("NULL pointer");
        if (s[2] == 1 && (!p[2] || !p[4] || !p[5])) return bad("stage 1 needs mean and the running statistics");
        kernel = TK_BN_FINALIZE;
        e = launch_bn_finalize(F(0), F(1), s[0], (int)s[1], F(2), F(3), F(4), F(5), (int)s[2], st);
    } else if (k == "bn_finalize_shifted") { // sizes M, C; scalar alpha; pointers stats, bias, mean, istd, running_mean, running_var, gamma, beta, tab
        if (s[0] < 1 || s[1] < 1 || !fits_int(s[1])) return bad("M < 1 or C < 1");
        for (int i = 0; i < 6; ++i)
            if (!p[i]) return bad("NULL pointer");
        if ((uintptr_t)p[0] % 8) return bad("stats is not 8-byte aligned");
        if (p[8] && (!p[6] || !p[7])) return bad("tab needs gamma and beta");
        kernel = TK_BN_FINALIZE_SHIFTED;
        e = launch_bn_finalize_shifted((double*)p[0], F(1), f[0], s[0], (int)s[1], F(2), F(3), F(4), F(5), F(6), F(7), F(8), st);
    } else if (k == "act_sums_finalize") {   // size C; scalar scale0; pointers stats, out0, out1, acc0, acc1
        if (s[0] < 1 || !fits_int(s[0])) return bad("C < 1");
        if (!p[0] || (uintptr_t)p[0] % 8) return bad("stats is NULL or not 8-byte aligned");
        kernel = TK_ACT_SUMS_FINALIZE;
        e = launch_act_sums_finalize((double*)p[0], (int)s[0], f[0], F(1), F(2), F(3), F(4), st);
    } else if (k == "act_table") {           // size n; pointers mu, istd, gamma, beta, dst
        if (s[0] < 1 || !fits_int(s[0])) return bad("n < 1");
        if (!p[4]) return bad("dst is NULL");
        if (p[0] ? (!p[1] || !p[2] || !p[3]) : (p[1] || p[2] || p[3])) return bad("the statistics are all set or all NULL");
        kernel = TK_ACT_TABLE;
        e = launch_act_table(F(0), F(1), F(2), F(3), (int)s[0], F(4), st);
    } else if (k == "sin_fwd") {             // sizes M, C, ldz, ldh; pointers Z, H, mu, istd, gamma, beta
        if (s[1] < 1 || !fits_int(s[1]) || s[2] < s[1] || s[3] < s[1]) return bad("C < 1 or a leading dimension below C");
        if (!p[0] || !p[1]) return bad("NULL pointer");
        if (p[2] ? (!p[3] || !p[4] || !p[5]) : (p[3] || p[4] || p[5])) return bad("the statistics are all set or all NULL");
        kernel = sin_fwd_choice(F(0), F(1), (int)s[1], s[2], s[3]);
        e = launch_sin_fwd(F(0), F(1), s[0], (int)s[1], s[2], s[3], F(2), F(3), F(4), F(5), st);
    } else if (k == "thin_dgrad") {          // sizes M, N, K, ldd, ldw, ldc, accumulate, eld; scalar alpha; pointers D, W, W3, C, ez, etab, emu, eistd, stats
        ThinDgradArgs a{};
        a.M = s[0]; a.N = (int)s[1]; a.K = (int)s[2]; a.ldd = s[3]; a.ldw = s[4]; a.ldc = s[5]; a.accumulate = (int)s[6]; a.eld = s[7]; a.alpha = f[0];
        a.D = F(0); a.W = F(1); a.W3 = F(2); a.C = F(3); a.ez = F(4); a.etab = F(5); a.emu = F(6); a.eistd = F(7); a.stats = (double*)p[8];
        if (s[2] < 1 || s[2] > 4) return bad("K must be 1..4");
        if (s[1] < 4 || s[1] > 1024 || a.ldd < a.K || a.ldw < a.N || a.ldc < a.N || s[6] > 1) return bad("N outside 4..1024, a leading dimension below its column count, or accumulate not 0 / 1");
        if (!a.D || !a.W || !a.C) return bad("NULL pointer");
        if (a.W3 && a.K != 4) return bad("W3 needs K = 4");
        if (a.ez && (a.eld < a.N || (uintptr_t)p[8] % 8 || !a.emu != !a.eistd)) return bad("the epilogue needs eld >= N, aligned sums and both or neither of emu / eistd");
        if (!a.ez && (a.etab || a.emu || a.eistd || a.stats)) return bad("epilogue arguments without ez");
        if (!thin_dgrad_ok(a)) return bad("thin_dgrad_ok refuses the shape (N, ldc, eld multiples of 4, 16-byte bases, table and sums with ez)");
        kernel = thin_dgrad_choice(a);
        e = launch_thin_dgrad(a, st);
    } else if (k == "wgrad") {               // sizes M, n_out, n_in, ldz, ldi, ldw, tab_cols, ldzz, M_global, route; scalars alpha, bias_alpha;
                                             // pointers dZ, In, dW, tab, z, gamma, mu, istd, sdy, sdyx, dbias
        const bool ride = p[4] != nullptr;
        if (s[9] > 1) return bad("route must be 1 (Rows) or 0 (exact fp32)");
        if (s[0] < 1 || s[1] < 1 || s[2] < 1 || !fits_int(s[1]) || !fits_int(s[2])) return bad("M, n_out or n_in < 1");
        if (!p[0] || !p[1] || !p[2]) return bad("dZ, In or dW is NULL");
        if (s[3] < s[1] || s[4] < s[2] || s[5] < s[2]) return bad("a leading dimension below its column count");
        if (s[3] >= (1 << 24) || s[4] >= (1 << 24) || (ride && s[7] >= (1 << 24))) return bad("a leading dimension of 2^24 or more (32-bit lane offsets over 64 rows)");
        if ((p[3] != nullptr) != (s[6] > 0) || s[6] > s[2]) return bad("the table needs 1 <= tab_cols <= n_in, tab_cols needs the table");
        for (int i = 5; i < 10; ++i)
            if ((p[i] != nullptr) != ride) return bad("the BatchNorm block (z, gamma, mu, istd, sdy, sdyx) is all set or all NULL");
        if (!ride && p[10]) return bad("dbias without the BatchNorm block");
        if (ride && (s[7] < s[1] || s[8] < s[0])) return bad("the BatchNorm block needs ldzz >= n_out (a leading dimension) and M_global >= M");
        if (s[9] == 0) return bad((ride || p[3]) ? "a table or a BatchNorm block needs the Rows route" : "the exact fp32 route has no kernel number: snerf_linear_wgrad runs it");
        // the ride writes dZ in place: one block over the inputs (bz = 1) per launch - the whole layer up to 256 inputs, the first 256 of a wider one (run_wgrad's split)
        if (ride && plan_wgrad_bf16x3(s[0], (int)s[1], s[2] > 256 ? 256 : (int)s[2], true, false).bz != 1) return bad("the BatchNorm ride needs bz = 1 and this layer cannot be split to get it");
        Product q;
        q.M = s[0]; q.n_out = (int)s[1]; q.n_in = (int)s[2]; q.alpha = f[0]; q.Y = F(0); q.ldy = s[3]; q.X = F(1); q.ldx = s[4]; q.dW = F(2); q.lddw = s[5];
        q.tab = F(3); q.tab_cols = (int)s[6];
        const WgradBN bn{F(4), s[7], F(5), F(6), F(7), F(8), F(9), 1.f / (float)s[8], f[1], F(10)};
        if (ride) q.bn = &bn;
        wgrad_note_begin();
        e = run_wgrad(q, Route::Rows, st);
        kernel = wgrad_note_end();
    } else if (k == "thin_wgrad") {          // sizes M, N, K, ldd, ldi, ldw, tab_cols; scalar alpha; pointers D, In, dW, dW3, tab
        ThinWgradArgs a{};
        a.M = s[0]; a.N = (int)s[1]; a.K = (int)s[2]; a.ldd = s[3]; a.ldi = s[4]; a.ldw = s[5]; a.tab_cols = (int)s[6]; a.tab_stride = a.tab_cols; a.alpha = f[0];
        a.D = F(0); a.In = F(1); a.dW = F(2); a.dW3 = F(3); a.tab = F(4);
        if (s[2] < 1 || s[2] > 4) return bad("K must be 1..4");
        if (s[0] < 1 || s[1] < 4 || s[1] > 1024 || a.ldd < a.K || a.ldi < a.N || a.ldw < a.N) return bad("M < 1, N outside 4..1024 or a leading dimension below its column count");
        if (!a.D || !a.In || !a.dW) return bad("D, In or dW is NULL");
        if (a.dW3 && a.K != 4) return bad("dW3 needs K = 4");
        if ((a.tab != nullptr) != (s[6] > 0) || s[6] > s[1]) return bad("the table needs 1 <= tab_cols <= N, tab_cols needs the table");
        if (!thin_wgrad_ok(a)) return bad("thin_wgrad_ok refuses the shape (N and ldi multiples of 4, In on 16 bytes)");
        kernel = thin_wgrad_choice(a);
        if (rows_dry_run()) return kernel;
        e = launch_thin_wgrad(a, st);
    } else if (k == "thin_fwd") {            // sizes M, N, K, ldi, ldw, ldo, tab_cols; scalar alpha; pointers In, W, W3, bias, bias3, Out, tab
        ThinFwdArgs a{};
        a.M = s[0]; a.N = (int)s[1]; a.K = (int)s[2]; a.ldi = s[3]; a.ldw = s[4]; a.ldo = s[5]; a.tab_cols = (int)s[6]; a.tab_stride = a.tab_cols; a.alpha = f[0];
        a.In = F(0); a.W = F(1); a.W3 = F(2); a.bias = F(3); a.bias3 = F(4); a.Out = F(5); a.tab = F(6);
        if (s[2] < 1 || s[2] > 4) return bad("K must be 1..4");
        if (s[0] < 1 || s[1] < 4 || s[1] > 256 || a.ldi < a.N || a.ldw < a.N || a.ldo < a.K) return bad("M < 1, N outside 4..256 or a leading dimension below its column count");
        if (!a.In || !a.W || !a.bias || !a.Out) return bad("In, W, bias or Out is NULL");
        if ((a.W3 || a.bias3) && a.K != 4) return bad("W3 and bias3 need K = 4");
        if ((a.tab != nullptr) != (s[6] > 0) || s[6] > s[1]) return bad("the table needs 1 <= tab_cols <= N, tab_cols needs the table");
        if (!thin_fwd_ok(a)) return bad("thin_fwd_ok refuses the shape (N and ldi multiples of 4, In on 16 bytes)");
        kernel = thin_fwd_choice(a);
        if (rows_dry_run()) return kernel;
        e = launch_thin_fwd(a, st);
    } else if (k == "point_out_fwd" || k == "point_out_bwd") {      // sizes n, n_samples, C; pointers in the order of PointOutArgs
        const bool bwd = k == "point_out_bwd";
        PointOutArgs a{};
        a.n = s[0]; a.n_samples = (int)s[1]; a.C = (int)s[2];
        a.head = F(0); a.adj = F(1); a.sv_raw = F(2); a.cls = F(3); a.rho = F(4); a.col = F(5); a.sv = F(6); a.adjust_col = F(7);
        a.d_rho = F(8); a.d_col = F(9); a.d_sv = F(10); a.d_head = F(11); a.d_adj = F(12); a.d_cls = F(13); a.d_sv_raw = F(14);
        if (s[1] < 1 || !fits_int(s[1])) return bad("n_samples < 1");
        if (!bwd) {
            if ((a.rho || a.col) && !a.head) return bad("rho and col need head");
            if (a.col && (s[2] < 1 || s[2] > 8 || !a.adj || !a.cls)) return bad("col needs 1 <= n_classes <= 8, adj and cls");
            if (a.adjust_col && !a.col) return bad("adjust_col needs col");
            if (a.sv && !a.sv_raw) return bad("sv needs sv_raw");
            if (!a.rho && !a.col && !a.sv) return bad("no output");
        } else {
            if (a.d_head && (s[2] < 1 || s[2] > 8 || !a.head || !a.adj || !a.cls)) return bad("d_head needs 1 <= n_classes <= 8, head, adj and cls");
            if (a.d_col && !a.col) return bad("d_col needs col");
            if ((a.d_adj || a.d_cls) && !a.d_head) return bad("d_adj and d_cls need d_head");
            if (!a.d_sv_raw != !a.d_sv || (a.d_sv && !a.sv)) return bad("d_sv_raw needs d_sv and sv");
            if (!a.d_head && !a.d_sv_raw) return bad("no output");
        }
        kernel = bwd ? TK_POINT_OUT_BWD : TK_POINT_OUT_FWD;
        e = launch_point_out(a, bwd, st);
    } else if (k == "softmax" || k == "softmax_bwd") {              // sizes rows, C; pointers x, p / p, dp, dx
        if (s[1] < 1 || !fits_int(s[1])) return bad("C < 1");
        for (int i = 0; i < d->np; ++i)
            if (!p[i]) return bad("NULL pointer");
        kernel = d->np == 2 ? TK_SOFTMAX : TK_SOFTMAX_BWD;
        e = d->np == 2 ? launch_softmax(F(0), F(1), s[0], (int)s[1], st) : launch_softmax_bwd(F(0), F(1), F(2), s[0], (int)s[1], st);
    } else if (k == "sigmoid" || k == "sigmoid_bwd") {              // size n; pointers x, y / y, dy, dx
        for (int i = 0; i < d->np; ++i)
            if (!p[i]) return bad("NULL pointer");
        kernel = d->np == 2 ? TK_SIGMOID : TK_SIGMOID_BWD;
        e = d->np == 2 ? launch_sigmoid(F(0), F(1), s[0], st) : launch_sigmoid_bwd(F(0), F(1), F(2), s[0], st);
    } else if (k == "colsum") {              // sizes M, C, ld; scalar alpha; pointers X, out
        if (s[1] < 1 || !fits_int(s[1]) || s[2] < s[1]) return bad("C < 1 or ld < C");
        if (!p[0] || !p[1]) return bad("NULL pointer");
        kernel = TK_COLSUM;
        e = launch_colsum(F(0), s[0], (int)s[1], s[2], f[0], F(1), st);
    } else if (k == "copy_cols") {           // sizes M, C, ld_src, ld_dst, accumulate; pointers src, dst
        if (s[1] < 1 || !fits_int(s[1]) || s[2] < s[1] || s[3] < s[1] || s[4] > 1) return bad("C < 1, a leading dimension below C, or accumulate not 0 / 1");
        if (!p[0] || !p[1]) return bad("NULL pointer");
        kernel = TK_COPY_COLS;
        e = launch_copy_cols(F(0), s[2], F(1), s[3], s[0], (int)s[1], s[4] != 0, st);
    } else if (k == "bcast_rows" || k == "reduce_rows") {           // sizes n (points) / n_groups, n_samples, C, ld of the per-point matrix, col0; pointers src, dst
        if (s[1] < 1 || !fits_int(s[1]) || s[2] < 1 || !fits_int(s[2]) || !fits_int(s[4]) || s[3] < s[4] + s[2]) return bad("n_samples < 1, C < 1 or ld < col0 + C");
        if (!p[0] || !p[1]) return bad("NULL pointer");
        kernel = k[0] == 'b' ? TK_BCAST_ROWS : TK_REDUCE_ROWS;
        e = k[0] == 'b' ? launch_bcast_rows(F(0), (int)s[2], F(1), s[3], (int)s[4], s[0], (int)s[1], st)
                        : launch_reduce_rows(F(0), s[3], (int)s[4], (int)s[2], F(1), s[0], (int)s[1], st);
    } else {                                 // fill_zero, copy_f32 (size: floats), fill_zero_bytes, copy_bytes (size: bytes); pointers dst [, src]
        for (int i = 0; i < d->np; ++i)
            if (!p[i]) return bad("NULL pointer");
        if (k == "fill_zero") { kernel = TK_FILL_ZERO; e = launch_fill_zero(F(0), s[0], st); }
        else if (k == "copy_f32") { kernel = TK_COPY_F32; e = launch_copy_f32(F(0), F(1), s[0], st); }
        else if (k == "fill_zero_bytes") { kernel = TK_FILL_ZERO_BYTES; e = launch_fill_zero_bytes(p[0], (size_t)s[0], st); }
        else { kernel = TK_COPY_BYTES; e = launch_copy_bytes(p[0], p[1], (size_t)s[0], st); }
    }
    if (e != hipSuccess) return snerf_set_error(SNERF_E_HIP, "snerf_train_kernel_debug: " + k + ": " + hipGetErrorString(e));
    return kernel;
}

// Introspection for tests: the row GEMMs' routing (rows_debug.h).
int snerf_rows_debug_set(const int* switches8, int dry_run, int x_padded) {
    if (switches8 && switches8[4] != 0 && switches8[4] != 2 && switches8[4] != 4 && switches8[4] != 8) return snerf_set_error(SNERF_E_INVALID, "snerf_rows_debug_set: pf must be 0, 2, 4 or 8");
    rows_debug_set(switches8, dry_run != 0, x_padded != 0);
    return SNERF_OK;
}
int snerf_rows_record_reset(int on) {
    rows_record_reset(on != 0);
    return SNERF_OK;
}
int snerf_rows_record_read(int32_t* host_out, int max_entries) {
    if (max_entries < 0 || (max_entries > 0 && !host_out)) return snerf_set_error(SNERF_E_INVALID, "snerf_rows_record_read: bad argument");
    return rows_record_read(host_out, max_entries);
}

// ---- the three products of a Linear layer as stand-alone calls (building blocks of the training engine; tests)
size_t snerf_linear_scratch_bytes(int n_out, int n_in) {
    const int64_t d = n_out > n_in ? n_out : n_in;
    return (size_t)(((d + 31) / 32) * ((d + 15) / 16) * 2048 + 256);
}

// a public call as a caller: bf16x3 from the first row on when asked for by `precision`; its dgrad never streams
static Policy public_policy(int precision) { return Policy{precision == 1, 1, true, false}; }
int snerf_linear_forward(int64_t n_points, int n_in, int n_out, const float* d_in, int64_t ld_in, const float* d_weight,
                         const float* d_bias, float alpha, float* d_out, int64_t ld_out, double* d_stats, int precision,
                         void* d_scratch, size_t scratch_bytes, const float* d_act_tab, int act_cols, void* stream) {
    if (n_points < 0 || n_in < 1 || n_out < 1) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_forward: bad shape");
    if (n_points == 0) return SNERF_OK;
    if (!d_in || !d_weight || !d_out || ld_in < n_in || ld_out < n_out) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_forward: bad argument");
    if (d_act_tab && (act_cols < 8 || act_cols % 8 || act_cols > n_in)) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_forward: act_cols must be a multiple of 8 within n_in");
    Product p;
    p.M = n_points; p.n_in = n_in; p.n_out = n_out; p.alpha = alpha; p.W = d_weight; p.bias = d_bias; p.frag = (const uint16_t*)d_scratch;
    p.X = d_in; p.ldx = ld_in; p.tab = d_act_tab; p.tab_cols = d_act_tab ? act_cols : 0; p.Y = d_out; p.ldy = ld_out; p.stats = d_stats;
    p.x_padded = rows_x_padded();      // snerf_rows_debug_set: the caller guarantees zero columns n_in .. next multiple of 16
    const Route r = route_fwd(p, public_policy(precision));
    if (r == Route::Rows && (!d_scratch || scratch_bytes < snerf_linear_scratch_bytes(n_out, n_in))) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_forward: scratch too small");
    if (r == Route::Fp32 && (d_stats || d_act_tab)) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_forward: column statistics / activation on load need the bf16x3 path");
    HIPCK(run_fwd(p, r, (hipStream_t)stream));
    return SNERF_OK;
}

int snerf_linear_dgrad(int64_t n_points, int n_in, int n_out, const float* d_grad_out, int64_t ld_go, const float* d_weight,
                       int n_cols, float alpha, int accumulate, float* d_grad_in, int64_t ld_gi, int precision, void* d_scratch,
                       size_t scratch_bytes, const float* d_below_z, int64_t ld_below_z, const float* d_below_tab,
                       const float* d_below_mu, const float* d_below_istd, double* d_sums, void* stream) {
    if (n_points < 0 || n_in < 1 || n_out < 1 || n_cols < 1 || n_cols > n_in) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_dgrad: bad shape");
    if (n_points == 0) return SNERF_OK;
    if (!d_grad_out || !d_weight || !d_grad_in || ld_go < n_out || ld_gi < n_cols) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_dgrad: bad argument");
    if (d_below_z && (!d_below_tab || !d_sums || ld_below_z < n_cols || (!d_below_mu) != (!d_below_istd)))
        return snerf_set_error(SNERF_E_INVALID, "snerf_linear_dgrad: the activation-backward epilogue needs table and sums");
    Product p;
    p.M = n_points; p.n_in = n_in; p.n_out = n_out; p.alpha = alpha; p.W = d_weight; p.Y = const_cast<float*>(d_grad_out); p.ldy = ld_go;      // (Y: read-only here)
    p.dX = d_grad_in; p.lddx = ld_gi; p.n_cols = n_cols; p.accumulate = accumulate != 0; p.frag = (const uint16_t*)d_scratch;
    p.x_padded = rows_x_padded();
    if (d_below_z) { p.below.z = d_below_z; p.below.ld = ld_below_z; p.below.tab = d_below_tab; p.below.mu = d_below_mu; p.below.istd = d_below_istd; p.below.sums = d_sums; }
    const Route r = route_dgrad(p, public_policy(precision));
    if (r == Route::Fp32 && d_below_z) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_dgrad: the activation-backward epilogue needs the bf16x3 path");
    if (r == Route::Rows && (!d_scratch || scratch_bytes < snerf_linear_scratch_bytes(n_out, n_in))) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_dgrad: scratch too small");
    HIPCK(run_dgrad(p, r, (hipStream_t)stream));
    return SNERF_OK;
}

int snerf_linear_wgrad(int64_t n_points, int n_in, int n_out, const float* d_grad_out, int64_t ld_go, const float* d_in,
                       int64_t ld_in, float alpha, float* d_grad_weight, int precision, const float* d_act_tab, int act_cols,
                       void* stream) {
    if (n_points < 0 || n_in < 1 || n_out < 1) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_wgrad: bad shape");
    if (n_points == 0) return SNERF_OK;
    if (!d_grad_out || !d_in || !d_grad_weight || ld_go < n_out || ld_in < n_in) return snerf_set_error(SNERF_E_INVALID, "snerf_linear_wgrad: bad argument");
    if (d_act_tab && (precision != 1 || act_cols < 1 || act_cols > n_in))
        return snerf_set_error(SNERF_E_INVALID, "snerf_linear_wgrad: activation on load needs the bf16x3 path and 1 <= act_cols <= n_in");
    Product p;
    p.M = n_points; p.n_in = n_in; p.n_out = n_out; p.alpha = alpha; p.dW = d_grad_weight; p.Y = const_cast<float*>(d_grad_out); p.ldy = ld_go;      // (Y: read-only without the BatchNorm option)
    p.X = d_in; p.ldx = ld_in; p.tab = d_act_tab; p.tab_cols = d_act_tab ? act_cols : 0;
    HIPCK(run_wgrad(p, route_wgrad(p, public_policy(precision)), (hipStream_t)stream));
    return SNERF_OK;
}

int snerf_trainer_set_allreduce(snerf_trainer* t, snerf_allreduce_fn fn, void* user, int world_size) {
    if (!t) return snerf_set_error(SNERF_E_INVALID, "NULL trainer");
    if (fn && world_size < 1) return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_set_allreduce: world_size must be >= 1");
    t->ar_fn = fn; t->ar_user = user; t->world = fn ? world_size : 1;
    return SNERF_OK;
}

int snerf_trainer_zero_grad(snerf_trainer* t, void* stream) {
    if (!t || !t->grads) return snerf_set_error(SNERF_E_STATE, "trainer not bound");
    HIPCK(snerf_zero_async(t->grads, 0, t->n_params * sizeof(float), (hipStream_t)stream));
    return SNERF_OK;
}

int snerf_trainer_adam_step(snerf_trainer* t, float lr, float beta1, float beta2, float eps, int step, void* stream) {
    if (!t || !t->params || !t->adam_m || !t->adam_v) return snerf_set_error(SNERF_E_STATE, "trainer not bound (Adam state)");
    if (step < 1) return snerf_set_error(SNERF_E_INVALID, "Adam step counts from 1");
    HIPCK(launch_adam(t->params, t->grads, t->adam_m, t->adam_v, t->n_params, lr, beta1, beta2, eps, step, (hipStream_t)stream));
    return SNERF_OK;
}

/* the same update with lr / betas / eps / bias corrections read from device memory: what a captured (hipGraph) training step launches */
int snerf_trainer_adam_step_dev(snerf_trainer* t, const float* d_hyper6, void* stream) {
    if (!t || !t->params || !t->adam_m || !t->adam_v) return snerf_set_error(SNERF_E_STATE, "trainer not bound (Adam state)");
    if (!d_hyper6) return snerf_set_error(SNERF_E_INVALID, "snerf_trainer_adam_step_dev: NULL hyper-parameter vector");
    HIPCK(launch_adam_dev(t->params, t->grads, t->adam_m, t->adam_v, t->n_params, d_hyper6, (hipStream_t)stream));
    return SNERF_OK;
}

/* The scalar terms of All_in_One_Eval.get_loss (Eval_Tools_2.py:340-450; solar rays on, default solar model) in two launches, with their weight vector, and
 * their gradients in one (see include/season_nerf_hip.h).  Every argument is checked before any launch. */
size_t snerf_loss_all_scratch_bytes(void) { return loss_all_scratch_bytes(); }
int snerf_loss_all_term_count(int flags) {
    if (flags < 0 || flags > 7) return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all: flags must be a combination of SNERF_LOSS_ADAPTIVE, SNERF_LOSS_PRIOR and SNERF_LOSS_SKY_DETACHED");
    return loss_all_idx(flags).n;
}
static int loss_all_args(LossAllArgs* a, const snerf_loss_in* in) {
    if (!in) return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all: NULL input description");
    if (snerf_loss_all_term_count(in->flags) < 0) return SNERF_E_INVALID;
    if (in->n_rays < 1 || in->n_solar_rays < 1 || in->n_samples < 1 || in->world < 1 || in->n_rays > 0x7fffffffll || in->n_solar_rays > (1ll << 40) / in->n_samples)
        return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all: ray / sample counts and world must be >= 1 (at most 2^31 - 1 image rays)");
    if (!in->d_rgb || !in->d_gt || !in->d_albedo || !in->d_sky || !in->d_solar_vis || !in->d_pv_exact || !in->d_pe_solar)
        return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all: NULL image-ray or sun-ray input");
    const bool ada = in->flags & SNERF_LOSS_ADAPTIVE, prior = in->flags & SNERF_LOSS_PRIOR;
    if (ada && (!in->d_alpha_color || !in->d_scale_color || !in->d_logz_value || !in->d_logz_slope))
        return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all: the adaptive colour loss needs alpha, scale and the log-partition table");
    if (prior && (!in->d_pe || !in->d_pe_supervised)) return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all: the prior phase needs PE and PE_Supervised");
    if (ada && prior && (!in->d_alpha_alpha || !in->d_scale_alpha))
        return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all: the adaptive loss in the prior phase needs the alpha loss object's alpha and scale");
    if (!(in->w_solar == in->w_solar) || !(in->w_color == in->w_color) || !(in->w_alpha == in->w_alpha)) return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all: NaN weight");
    *a = LossAllArgs{in->n_rays, in->n_solar_rays, in->n_samples, in->flags, in->d_rgb, in->d_rgb_merged, in->d_gt, in->d_albedo, in->d_sky, in->d_solar_vis, in->d_pv_exact,
                     in->d_pe_solar, prior ? in->d_pe : nullptr, prior ? in->d_pe_supervised : nullptr, ada ? in->d_alpha_color : nullptr, ada ? in->d_scale_color : nullptr,
                     (ada && prior) ? in->d_alpha_alpha : nullptr, (ada && prior) ? in->d_scale_alpha : nullptr, ada ? in->d_logz_value : nullptr,
                     ada ? in->d_logz_slope : nullptr, in->d_albedo_min_global, in->d_albedo_min_global ? in->world : 1, in->w_solar, in->w_color, in->w_alpha};
    return SNERF_OK;
}
int snerf_loss_all_forward(const snerf_loss_in* in, void* d_scratch, float* d_vals, float* d_weights, float* d_aux14, void* stream) {
    LossAllArgs a;
    RC(loss_all_args(&a, in));
    if (!d_scratch || !d_vals || !d_weights || !d_aux14) return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all_forward: NULL scratch or output");
    HIPCK(launch_loss_all(a, d_scratch, d_vals, d_weights, d_aux14, (hipStream_t)stream));
    return SNERF_OK;
}
int snerf_loss_all_backward(const snerf_loss_in* in, const float* d_aux14, const float* d_g_vals, const snerf_loss_grads* out, void* stream) {
    LossAllArgs a;
    RC(loss_all_args(&a, in));
    if (!d_aux14 || !d_g_vals || !out) return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all_backward: NULL aux, upstream gradient or output description");
    const bool ada = in->flags & SNERF_LOSS_ADAPTIVE, prior = in->flags & SNERF_LOSS_PRIOR;
    if (!out->d_g_rgb || !out->d_g_albedo || !out->d_g_sky || !out->d_g_solar_vis || (a.rgb_merged && !out->d_g_rgb_merged) || (prior && !out->d_g_pe) ||
        (ada && (!out->d_g_alpha_color || !out->d_g_scale_color)) || (ada && prior && (!out->d_g_alpha_alpha || !out->d_g_scale_alpha)))
        return snerf_set_error(SNERF_E_INVALID, "snerf_loss_all_backward: NULL gradient output for an input this configuration differentiates");
    const LossAllGrads G{out->d_g_rgb, out->d_g_rgb_merged, out->d_g_albedo, out->d_g_sky, out->d_g_solar_vis, out->d_g_pe, out->d_g_alpha_color, out->d_g_scale_color,
                         out->d_g_alpha_alpha, out->d_g_scale_alpha};
    HIPCK(launch_loss_all_bwd(a, d_g_vals, d_aux14, G, (hipStream_t)stream));
    return SNERF_OK;
}

/* the same update on caller-owned arenas (no trainer object): what season_nerf::fused_adam_ binds */
int snerf_adam_step(float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2, float eps,
                    int step, void* stream) {
    if (n < 0 || (n && (!d_params || !d_grads || !d_m || !d_v))) return snerf_set_error(SNERF_E_INVALID, "snerf_adam_step: bad argument");
    if (step < 1) return snerf_set_error(SNERF_E_INVALID, "Adam step counts from 1");
    if (n == 0) return SNERF_OK;
    HIPCK(launch_adam(d_params, d_grads, d_m, d_v, n, lr, beta1, beta2, eps, step, (hipStream_t)stream));
    return SNERF_OK;
}

}  // extern "C"
