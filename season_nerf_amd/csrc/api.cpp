// C ABI of include/season_nerf_hip.h.  Host logic only: argument checking, model object, launch sequencing.
#include "../../include/season_nerf_hip.h"

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>

#include "kernels.h"
#include "loader_common.h"
#include "pack.h"
#include "train.h"

#ifndef SNERF_I8_BUDGET
#define SNERF_I8_BUDGET 1.0e-4
#endif

using namespace snerf;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}
int snerf_set_error(int code, const std::string& msg) { return fail(code, msg); }   // used by train.cpp
static int fail_hip(hipError_t e, const char* what) {
    return fail(SNERF_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
static int fail_pack(const std::string& err) {      // what the packer and the error model report: a tensor that is not there, or one of the wrong shape
    return fail(err.rfind("missing", 0) == 0 ? SNERF_E_MISSING : SNERF_E_INVALID, err);
}

// A/B switches of the environment, read once per process
struct Switches {
    bool i8_one_wave;             // SNERF_I8_ONE_WAVE=1: the one-wave int8 kernel (kernels_i8.hip) where the two-wave kernel would run
    bool i8x2_mfma32;             // SNERF_I8X2_MFMA32=1: the two-wave kernel's 32x32x32 code and stream where its 16x16x64 instances would run
    bool group_f32;               // SNERF_GROUP_F32=1: width 512, the per-ray networks in the exact-fp32 layer-wise form of rounds 3-5
    bool group_one_wave;          // SNERF_GROUP_ONE_WAVE=1: snerf_set_group_kernel starts at 1
    bool rayvis_no_early_out;     // SNERF_RAYVIS_NO_EARLY_OUT=1: ray visibility walks every pass of every ray (mlp_device.h raysum_saturated)
    bool rayvis_sun_first;        // SNERF_RAYVIS_SUN_FIRST=1: ... its passes in the order before round 6's reversal
};
static const Switches& switches() {
    const auto on = [](const char* name) { return getenv(name) != nullptr; };
    static const Switches s{on("SNERF_I8_ONE_WAVE"), on("SNERF_I8X2_MFMA32"), on("SNERF_GROUP_F32"), on("SNERF_GROUP_ONE_WAVE"), on("SNERF_RAYVIS_NO_EARLY_OUT"),
                            on("SNERF_RAYVIS_SUN_FIRST")};
    return s;
}

// The packed programs of a model, under the program numbers of snerf_model_pack_host
enum : int {
    P_FIELD = PROG_FIELD,      // field network, bf16 pairs in the canonical order (kernels.hip: widths 64, 256)
    P_GROUP = PROG_GROUP,      // per-ray (time / sun) networks, likewise
    P_I8 = 2,                  // field network in the int8-digit format (SNERF_PREC_I8X3 only)
    P_KS = 3,                  // P_FIELD in the K-split order of kernels_ks.hip (width 512)
    P_KSG = 4,                 // P_GROUP in the same order: width 512 under every precision (round 6; exact fp32 layer by layer before)
    P_K64 = 5,                 // P_I8's digits in the layout of v_mfma_i32_16x16x64_i8 (program.h "k64": what kernels_i8x2.hip runs at W = 256)
    P_NUM = 6
};
struct ProgramSlot {
    Packed host;
    uint8_t* d_stream = nullptr;      // device copies, made by snerf_model_finalize of the programs the model launches
    float* d_table = nullptr;         // bias table (bf16 programs) / scale, bias and raw-coordinate tables (int8 digits)
};

struct snerf_model {
    int W = 0, C = 0;
    int precision = SNERF_PREC_BF16X3;
    bool auto_mode = false;          // SNERF_PREC_AUTO was asked for: `precision` holds the resolved mode once `resolved`
    bool resolved = true;
    bool have_estimate = false;      // the error model of the current tensors (computed once: ~10 ms of host time at W = 256, ~40 at 512)
    snerf_i8_estimate estimate{};
    Weights w;
    bool finalized = false;
    ProgramSlot prog[P_NUM];
    // Widths without a bf16 group kernel (512): the per-ray networks (time -> class softmax, sun -> sky colour: one row per ray,
    // 1/S of the field network's work) run layer by layer in exact fp32 (v_mfma_f32_32x32x2_f32, csrc/gemm.hip) - their error is
    // not averaged over a ray's samples, so they get the full precision.  Device copy of the five layers' fp32 weights:
    float* d_group_f32 = nullptr;
    size_t g32_off[10] = {0};        // weight / bias offsets (floats) of time_layer_1, time_layer_2, get_class_layer, fc_sky_color_1, fc_sky_color_2
    // sun walk: device copy of the walk stream (program.h sun_walk_*) of the most recent n_suns, built at the first snerf_field_sun_walk_rays that asks for it
    mutable uint8_t* d_walk = nullptr;
    mutable int walk_suns = 0;
    int n_cu = 0;
};

static void release(ProgramSlot& s) {
    if (s.d_stream) (void)hipFree(s.d_stream);
    if (s.d_table) (void)hipFree(s.d_table);
    s.d_stream = nullptr;
    s.d_table = nullptr;
}
// device copy of a packed program; one that an earlier, failed snerf_model_finalize left stays, a failure here leaves none behind
static int upload(ProgramSlot& s) {
    if (s.d_stream) return SNERF_OK;
    const size_t stream_bytes = s.host.stream.size(), table_bytes = s.host.bias.size() * 4;
    const char* what = "hipMalloc";
    hipError_t e = hipMalloc((void**)&s.d_stream, stream_bytes);
    if (e == hipSuccess) e = hipMalloc((void**)&s.d_table, table_bytes);
    if (e == hipSuccess) {
        what = "hipMemcpy";
        e = hipMemcpy(s.d_stream, s.host.stream.data(), stream_bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(s.d_table, s.host.bias.data(), table_bytes, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) return SNERF_OK;
    release(s);
    return fail_hip(e, what);
}

struct snerf_loader {
    const float* d_table = nullptr;
    int64_t n = 0, batch = 0, bpe = 0;      // rows of the table, rows per batch, batches per epoch
    uint64_t seed = 0;
    int drop_last = 0, rank = 0, world = 1, bits = 2;
    float b[6] = {0};                        // x0, dx, y0, dy, z_lo, z_hi of the sun-check rays
    int64_t* d_state = nullptr;              // {epoch, batch_in_epoch, draws, reserved}: what the kernels read
    int64_t shadow[4] = {0, 0, 0, 0};        // host copy, advanced per uncaptured launch: sizes a short last batch, nothing else
};

struct snerf_step_inputs {
    uint64_t seed = 0;
    int64_t n_rays = 0, n_samples = 0, table_rows = 0;
    int rank = 0;
    double H[12] = {0}, wc[3] = {0}, lon_scale = 0;
    const float* d_table = nullptr;          // [table_rows, 8], the caller's
    int64_t* d_state = nullptr;              // {draws, step, reserved, reserved}: what the kernels read; allocated by the first draw
    int64_t shadow[4] = {0, 0, 0, 0};        // host copy, advanced per uncaptured launch
};

extern "C" {

const char* snerf_last_error(void) { return g_err.c_str(); }
int snerf_abi_version(void) { return 10; }

snerf_model* snerf_model_create(int layer_width, int n_classes) {
    if (layer_width != 64 && layer_width != 256 && layer_width != 512) {
        fail(SNERF_E_INVALID, "layer_width " + std::to_string(layer_width) +
                                  " has no compiled kernel (built widths: 64, 256, 512)");
        return nullptr;
    }
    if (n_classes < 1 || n_classes > kMaxClasses) {
        fail(SNERF_E_INVALID, "n_classes must be in [1," + std::to_string(kMaxClasses) + "]");
        return nullptr;
    }
    snerf_model* m = new snerf_model();
    m->W = layer_width;
    m->C = n_classes;
    return m;
}

int snerf_model_set_precision(snerf_model* m, int precision) {
    if (!m) return fail(SNERF_E_INVALID, "NULL model");
    if (m->finalized) return fail(SNERF_E_STATE, "model already finalized (set the precision before snerf_model_finalize)");
    if (precision != SNERF_PREC_BF16X3 && precision != SNERF_PREC_BF16 && precision != SNERF_PREC_I8X3 && precision != SNERF_PREC_AUTO)
        return fail(SNERF_E_INVALID, "unknown precision mode " + std::to_string(precision));
    m->auto_mode = precision == SNERF_PREC_AUTO;
    m->resolved = !m->auto_mode;
    m->precision = precision;
    return SNERF_OK;
}
int snerf_model_precision(const snerf_model* m) { return m ? m->precision : -1; }

// Budget of the int8 error model (pack.cpp estimate_i8): the predicted relative error of the rendered colour, which the model
// puts at about twice the observed worst case.  Calibration: tools/calibrate_i8_bound.py (CPU emulation of the digit arithmetic
// against fp64 on init-law, outlier, heavy-tailed and high-gain weight sets at W = 64 / 256 / 512): colour and depth stay below
// 5e-5 relative wherever the prediction is below this value; the GPU kernels are held to it against the reference itself in
// tests/test_gpu_stress.py.
static const double kI8Budget = SNERF_I8_BUDGET;

static int i8_estimate(snerf_model* m, snerf_i8_estimate* out) {
    if (m->have_estimate) { *out = m->estimate; return SNERF_OK; }
    I8Estimate e;
    std::string err;
    if (!estimate_i8(m->w, m->W, m->C, &e, &err)) return fail_pack(err);
    for (int i = 0; i < 4; ++i) out->head_rms[i] = e.head_rms[i];
    out->hidden_rms = e.hidden_rms;
    out->worst = e.worst;
    out->rgb_pred = e.rgb_pred;
    out->budget = kI8Budget;
    out->acc_bound = e.acc_bound;
    out->ok = (e.rgb_pred <= kI8Budget && e.acc_bound < (1LL << 31)) ? 1 : 0;
    m->estimate = *out;
    m->have_estimate = true;
    return SNERF_OK;
}

int snerf_model_i8_estimate(snerf_model* m, snerf_i8_estimate* out) {
    if (!m || !out) return fail(SNERF_E_INVALID, "snerf_model_i8_estimate: NULL argument");
    return i8_estimate(m, out);
}

int snerf_model_set_tensor(snerf_model* m, const char* key, const float* host_data, size_t numel) {
    if (!m || !key || (!host_data && numel)) return fail(SNERF_E_INVALID, "snerf_model_set_tensor: NULL argument");
    if (m->finalized) return fail(SNERF_E_STATE, "model already finalized");
    Tensor t;
    t.data.assign(host_data, host_data + numel);
    m->w.t[key] = std::move(t);
    m->have_estimate = false;
    return SNERF_OK;
}

static bool bf16_width(int W) { return W == 64 || W == 256; }     // widths the bf16 kernels (kernels.hip) are instantiated for
static bool ks_width(int W) { return W == 512; }                  // ... the K-split bf16x3 field kernel (kernels_ks.hip): the reference's default width

// Which programs a model of this width and (resolved) precision holds.  Without `want_bf16_field`: the ones it launches, which snerf_model_finalize uploads.
// With it (snerf_model_pack_host, the sun walk's stream): also the bf16 field program where the model itself runs int8 digits.
static bool program_needed(const snerf_model* m, int p, bool want_bf16_field) {
    const bool i8 = m->precision == SNERF_PREC_I8X3;
    switch (p) {
        case P_FIELD: return bf16_width(m->W) && (!i8 || want_bf16_field);
        case P_GROUP: return bf16_width(m->W);
        case P_I8: return i8;
        case P_KS: return ks_width(m->W) && (m->precision == SNERF_PREC_BF16X3 || want_bf16_field);
        case P_KSG: return ks_width(m->W);      // bf16x3 on the wave-pair structure, whatever the field's mode
        case P_K64: return i8 && i8x2_k64_built(m->W, 0);      // the two-wave kernel's instances on the 16x16x64 shape read their own stream
    }
    return false;
}

static int pack_both(snerf_model* m, bool want_bf16_field = false) {
    if (!m->resolved) {          // SNERF_PREC_AUTO: int8 digits where their error bound holds for these weights
        snerf_i8_estimate e;
        int rc = i8_estimate(m, &e);
        if (rc) return rc;
        m->precision = e.ok ? SNERF_PREC_I8X3 : SNERF_PREC_BF16X3;
        m->resolved = true;
    }
    if (m->precision == SNERF_PREC_I8X3 && !m->auto_mode) {      // an explicit request is honoured, but never past the integer range
        snerf_i8_estimate e;
        int rc = i8_estimate(m, &e);
        if (rc) return rc;
        if (e.acc_bound >= (1LL << 31))
            return fail(SNERF_E_INVALID, "SNERF_PREC_I8X3: a weight row of this model can overflow the int32 accumulators (bound " +
                                             std::to_string((long long)e.acc_bound) + " >= 2^31); use SNERF_PREC_AUTO or SNERF_PREC_BF16X3");
    }
    if (!bf16_width(m->W) && m->precision != SNERF_PREC_I8X3 && !(ks_width(m->W) && m->precision == SNERF_PREC_BF16X3))
        return fail(SNERF_E_INVALID, "layer_width " + std::to_string(m->W) + " has fused kernels only under SNERF_PREC_I8X3 and SNERF_PREC_BF16X3");
    static const int order[P_NUM] = {P_KS, P_KSG, P_FIELD, P_GROUP, P_I8, P_K64};      // decides which error a model with several defects reports
    for (int p : order) {
        if (!program_needed(m, p, want_bf16_field)) continue;
        // the K-split programs are permutations of a canonical one, which stays on the host where snerf_model_pack_host can ask for it: the per-ray
        // networks always, the field network (11 MB) on request
        const int canon = p == P_KS ? P_FIELD : p == P_KSG ? P_GROUP : -1;
        const bool keep_canon = canon == P_GROUP || (canon == P_FIELD && want_bf16_field);
        if (!m->prog[p].host.stream.empty() && !(keep_canon && m->prog[canon].host.stream.empty())) continue;
        std::string err;
        Packed out, tmp;
        const bool ok = canon >= 0 ? pack_program(m->w, canon, m->W, m->C, /*fold_bn=*/true, &tmp, &err) && permute_program_ks(tmp, m->W, m->C, &out, &err, canon)
                      : p == P_I8  ? pack_program_i8(m->w, PROG_FIELD, m->W, m->C, /*fold_bn=*/true, &out, &err)
                      : p == P_K64 ? pack_program_k64(m->w, m->W, m->C, /*fold_bn=*/true, &out, &err)
                                   : pack_program(m->w, p, m->W, m->C, /*fold_bn=*/true, &out, &err);
        if (!ok) return fail_pack(err);
        m->prog[p].host = std::move(out);
        if (keep_canon) m->prog[canon].host = std::move(tmp);
    }
    return SNERF_OK;
}

int snerf_model_resolve_precision(snerf_model* m) {
    if (!m) return fail(SNERF_E_INVALID, "NULL model");
    int rc = pack_both(m);
    return rc ? rc : m->precision;
}

int snerf_model_pack_host(snerf_model* m, int program, uint8_t* stream_out, size_t* stream_bytes, float* bias_out,
                          size_t* bias_floats) {
    if (!m || program < 0 || program > 5) return fail(SNERF_E_INVALID, "snerf_model_pack_host: bad argument");
    if (program == 5 && (m->precision != SNERF_PREC_I8X3 || !i8x2_k64_built(m->W, 0)))
        return fail(SNERF_E_STATE, "program 5 (int8 digits for the 16x16x64 matrix instruction) exists only under SNERF_PREC_I8X3 at width 256");
    if (program == 2 && m->precision != SNERF_PREC_I8X3)
        return fail(SNERF_E_STATE, "program 2 (int8-digit field network) exists only under SNERF_PREC_I8X3");
    if (program == 3 && !ks_width(m->W)) return fail(SNERF_E_STATE, "program 3 (K-split bf16 field network) exists only at width 512");
    if (program == 4 && !ks_width(m->W)) return fail(SNERF_E_STATE, "program 4 (K-split per-ray networks) exists only at width 512");
    int rc = pack_both(m, program == P_FIELD || program == P_KS);
    if (rc) return rc;
    const Packed& P = m->prog[program].host;
    if (stream_bytes) *stream_bytes = P.stream.size();
    if (bias_floats) *bias_floats = P.bias.size();
    if (stream_out) std::memcpy(stream_out, P.stream.data(), P.stream.size());
    if (bias_out) std::memcpy(bias_out, P.bias.data(), P.bias.size() * 4);
    return SNERF_OK;
}

int snerf_model_finalize(snerf_model* m) {
    if (!m) return fail(SNERF_E_INVALID, "NULL model");
    if (m->finalized) return SNERF_OK;
    int rc = pack_both(m);
    if (rc) return rc;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return fail_hip(e, "hipGetDevice (is a GPU visible?)");
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return fail_hip(e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SNERF_E_HIP, std::string("this library is built for gfx950 only, device is ") + prop.gcnArchName);
    m->n_cu = prop.multiProcessorCount;
    for (int p = 0; p < P_NUM; ++p)      // the programs this model launches (a bf16 field program packed on request under int8 digits stays on the host)
        if (program_needed(m, p, false) && (rc = upload(m->prog[p])) != SNERF_OK) return rc;
    if (!bf16_width(m->W)) {      // fp32 weights of the per-ray networks
        static const char* keys[5] = {"time_layer_1.linear", "time_layer_2.linear", "get_class_layer", "G_NeRF_net.fc_sky_color_1.linear",
                                      "G_NeRF_net.fc_sky_color_2"};
        std::vector<float> blob;
        for (int i = 0; i < 5; ++i)
            for (int j = 0; j < 2; ++j) {
                const std::string k = std::string(keys[i]) + (j ? ".bias" : ".weight");
                const Tensor* t = m->w.find(k);
                if (!t) return fail(SNERF_E_MISSING, "missing tensor: " + k);
                m->g32_off[2 * i + j] = blob.size();
                blob.insert(blob.end(), t->data.begin(), t->data.end());
                blob.resize((blob.size() + 3) / 4 * 4, 0.f);           // 16-byte aligned rows for the GEMM's vector loads
            }
        const int W = m->W, C = m->C, W4 = W / 4;
        const size_t want[10] = {(size_t)W * 10, (size_t)W, (size_t)W * W, (size_t)W, (size_t)C * W, (size_t)C, (size_t)W4 * 27, (size_t)W4, (size_t)3 * W4, 3};
        for (int i = 0; i < 10; ++i) {
            const size_t have = (i < 9 ? m->g32_off[i + 1] : blob.size()) - m->g32_off[i];
            if (have < want[i] || have >= want[i] + 4) return fail(SNERF_E_INVALID, std::string("tensor of ") + keys[i / 2] + " has the wrong size");
        }
        if ((e = hipMalloc((void**)&m->d_group_f32, blob.size() * 4)) != hipSuccess) return fail_hip(e, "hipMalloc");
        if ((e = hipMemcpy(m->d_group_f32, blob.data(), blob.size() * 4, hipMemcpyHostToDevice)) != hipSuccess) return fail_hip(e, "hipMemcpy");
    }
    m->finalized = true;
    return SNERF_OK;
}

void snerf_model_destroy(snerf_model* m) {
    if (!m) return;
    for (ProgramSlot& s : m->prog) release(s);
    if (m->d_group_f32) (void)hipFree(m->d_group_f32);
    if (m->d_walk) (void)hipFree(m->d_walk);
    delete m;
}

int snerf_model_width(const snerf_model* m) { return m ? m->W : 0; }
int snerf_model_classes(const snerf_model* m) { return m ? m->C : 0; }

static int check_ready(const snerf_model* m) {
    if (!m) return fail(SNERF_E_INVALID, "NULL model");
    if (!m->finalized) return fail(SNERF_E_STATE, "model not finalized (call snerf_model_finalize)");
    return SNERF_OK;
}
// ... for the walk kernels, which exist for the bf16x3 field program only; `what`: "<the kernels> exist", as the message of entry point `fn` names them
static int check_walk_model(const snerf_model* m, const char* fn, const char* what) {
    int rc = check_ready(m);
    if (rc) return rc;
    if (m->precision != SNERF_PREC_BF16X3 || !(bf16_width(m->W) || ks_width(m->W)))
        return fail(SNERF_E_INVALID, std::string(fn) + ": the " + what + " for SNERF_PREC_BF16X3 at widths 64, 256 and 512 only");
    return SNERF_OK;
}

// time -> class softmax (T_NeRF_net_v2.py:77-78,160-163) and sun -> sky colour (G_NeRF.py:110-111) layer by layer in exact fp32:
// encodings (misc.py:105-139), SineLayer = sin(30 (x W^T + b)) (misc.py:188-189), Linear.  Scratch is stream-ordered.
static int group_forward_f32(const snerf_model* m, int64_t R, const float* d_time, const float* d_sun, float* d_classes, float* d_sky_raw,
                             float* d_sky, hipStream_t st) {
    const int W = m->W, C = m->C, W4 = W / 4;
    const size_t per_ray = 12 + (size_t)2 * W + 8 + 28 + W4 + 4;
    float* ws = nullptr;
    hipError_t e = hipMallocAsync((void**)&ws, per_ray * (size_t)R * 4, st);
    if (e != hipSuccess) return fail_hip(e, "hipMallocAsync (per-ray network scratch)");
    float *pe_t = ws, *h1 = pe_t + 12 * R, *h2 = h1 + (size_t)W * R, *logits = h2 + (size_t)W * R, *pe_s = logits + 8 * R, *k1 = pe_s + 28 * R,
          *sky_raw = k1 + (size_t)W4 * R;
    const float* P = m->d_group_f32;
    auto linear = [&](int layer, const float* in, int64_t ld_in, int K, float* out, int64_t ld_out, int N, float alpha) {
        GemmArgs g{};
        g.A = in; g.B = P + m->g32_off[2 * layer]; g.C = out;
        g.M = R; g.N = N; g.K = K;
        g.sAm = ld_in; g.sAk = 1; g.sBk = 1; g.sBn = K; g.ldc = ld_out;
        g.alpha = alpha; g.bias = P + m->g32_off[2 * layer + 1]; g.colsum = nullptr; g.flags = 0; g.splitk = 1;
        return launch_gemm(g, st);
    };
#define GF(x) do { if ((e = (x)) != hipSuccess) { (void)hipFreeAsync(ws, st); return fail_hip(e, "per-ray network (fp32)"); } } while (0)
    if (d_classes) {
        GF(launch_pe_small(d_time, 4, 2, PE_TIME_N, R, pe_t, 12, st));
        GF(linear(0, pe_t, 12, PE_TIME_F, h1, W, W, 30.f));
        GF(launch_sin_fwd(h1, h1, R, W, W, W, nullptr, nullptr, nullptr, nullptr, st));
        GF(linear(1, h1, W, W, h2, W, W, 30.f));
        GF(launch_sin_fwd(h2, h2, R, W, W, W, nullptr, nullptr, nullptr, nullptr, st));
        GF(linear(2, h2, W, W, logits, C, C, 1.f));
        GF(launch_softmax(logits, d_classes, R, C, st));
    }
    if (d_sky_raw || d_sky) {
        float* raw = d_sky_raw ? d_sky_raw : sky_raw;
        GF(launch_pe_small(d_sun, 3, 3, PE_SUN_N, R, pe_s, 28, st));
        GF(linear(3, pe_s, 28, PE_SUN_F, k1, W4, W4, 30.f));
        GF(launch_sin_fwd(k1, k1, R, W4, W4, W4, nullptr, nullptr, nullptr, nullptr, st));
        GF(linear(4, k1, W4, W4, raw, 3, 3, 1.f));
        if (d_sky) GF(launch_sigmoid(raw, d_sky, R * 3, st));
    }
#undef GF
    e = hipFreeAsync(ws, st);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "hipFreeAsync");
}

// ---- what a launch reads: one place decides the stream, its tables and the kernel
static void set_program(MlpArgs& a, const ProgramSlot& s, size_t stream_bytes) {      // stream_bytes: the part of the stream a tile cycles over
    a.stream = s.d_stream;
    a.stream_bytes = (uint32_t)stream_bytes;
    a.bias = s.d_table;
    a.bias_floats = (int)s.host.bias.size();
}
static snerf_field_out_dev to_dev(const snerf_field_out* out) {
    return {out->d_rho, out->d_solar_vis, out->d_col_raw, out->d_adjust, out->d_col, out->d_adjust_col, out->d_points, nullptr};
}
// the ray part of the arguments: n points or rays, each group_size of them sharing a sun / classes row
static MlpArgs ray_args(const snerf_model* m, int64_t n, const float* d_top, const float* d_bot, const float* d_tvals, int n_samples, int64_t group_size,
                        int ray_flags) {
    MlpArgs a{};
    a.n = n;
    a.n_classes = m->C;
    a.top = d_top;
    a.bot = d_bot;
    a.tvals = d_tvals;
    a.n_samples = n_samples;
    a.group_size = group_size;
    a.ray_flags = ray_flags;
    return a;
}

// the field program in bf16 pairs, in the order this width's kernels read it (the sun walk's stream is cut from its host copy under every precision)
static const ProgramSlot& bf16_field(const snerf_model* m) { return m->prog[ks_width(m->W) ? P_KS : P_FIELD]; }

enum FieldKernel { K_BF16, K_KS, K_I8, K_I8X2 };      // kernels.hip (bf16x3 and the bf16 fast mode), kernels_ks.hip, kernels_i8.hip, kernels_i8x2.hip
struct FieldRoute {
    FieldKernel kernel;
    const ProgramSlot* slot;
    int chunks;                            // chunks per tile: the layers of the variant
    int k64;                               // the slot is P_K64
    int tile_points, block, lds_bytes;     // what snerf_field_kernel_info reports
};
// Which kernel and which program a field launch of this model gets.  Works on an un-finalized model whose programs are packed; the walk kernels
// (bf16x3 models only) take slot and chunks from here too.
static FieldRoute field_route(const snerf_model* m, int variant) {
    const int W = m->W, C = m->C;
    FieldRoute r{};
    if (m->precision == SNERF_PREC_I8X3) {
        // two waves per SIMD wherever the activations leave room for it; their instances built on v_mfma_i32_16x16x64_i8 (W = 256) read the k64 stream
        const bool two_waves = W <= 256 && !switches().i8_one_wave;
        r.kernel = two_waves ? K_I8X2 : K_I8;
        r.k64 = two_waves && !switches().i8x2_mfma32 && !m->prog[P_K64].host.stream.empty() && i8x2_k64_built(W, variant);
        r.slot = &m->prog[r.k64 ? P_K64 : P_I8];
        r.chunks = r.k64 ? k64_chunk_start(W, C, field_variant_layers(variant)) : field_variant_chunks_i8(W, C, variant);
        r.tile_points = two_waves ? 256 : mlp_tile_points();
        r.block = two_waves ? 512 : 256;
        r.lds_bytes = (W > 256 ? 5 : 7) * kChunkBytes + (int)r.slot->host.bias.size() * 4 + kVoteBytes;
        return r;
    }
    const bool ks = ks_width(W);      // 64 points per tile (two wave pairs)
    r.kernel = ks ? K_KS : K_BF16;
    r.slot = &bf16_field(m);
    r.chunks = ks ? field_variant_chunks_ks(W, C, variant) : field_variant_chunks(W, C, variant);
    r.tile_points = ks ? mlp_ks_tile_points() : mlp_tile_points();
    r.block = 256;
    r.lds_bytes = ks ? mlp_ks_lds_bytes((int)r.slot->host.bias.size()) : mlp_lds_bytes((int)r.slot->host.bias.size());
    return r;
}
static void set_program(MlpArgs& a, const FieldRoute& r) {
    set_program(a, *r.slot, (size_t)r.chunks * kChunkBytes);
    a.k64 = r.k64;
}

// 0: kernels_group.hip (output blocks split over the waves), 1: kernels.hip (one wave per 32 rays); SNERF_GROUP_ONE_WAVE=1: start at 1 (A/B)
static std::atomic<int>& group_kernel_mode() {
    static std::atomic<int> mode{switches().group_one_wave ? 1 : 0};
    return mode;
}
int snerf_set_group_kernel(int mode) {
    if (mode != 0 && mode != 1) return fail(SNERF_E_INVALID, "snerf_set_group_kernel: mode must be 0 (split) or 1 (one wave)");
    group_kernel_mode().store(mode);
    return SNERF_OK;
}

int snerf_group_forward(const snerf_model* m, int64_t n_groups, const float* d_time, const float* d_sun,
                        float* d_classes, float* d_sky_raw, float* d_sky, void* stream) {
    int rc = check_ready(m);
    if (rc) return rc;
    if (n_groups == 0) return SNERF_OK;
    if (n_groups < 0 || !d_time || !d_sun) return fail(SNERF_E_INVALID, "snerf_group_forward: bad argument");
    // width 512: the wave-pair kernel (bf16x3, as the per-ray networks of the other widths); SNERF_GROUP_F32=1: the exact-fp32 layer-wise form of rounds 3-5 (A/B)
    const bool ks = ks_width(m->W);
    const ProgramSlot& s = m->prog[ks ? P_KSG : P_GROUP];
    if (m->d_group_f32 && (switches().group_f32 || !s.d_stream)) return group_forward_f32(m, n_groups, d_time, d_sun, d_classes, d_sky_raw, d_sky, (hipStream_t)stream);
    MlpArgs a{};
    set_program(a, s, ks ? (size_t)group_chunks_ks(m->W, m->C) * kChunkBytes : s.host.stream.size());
    a.n = n_groups;
    a.n_classes = m->C;
    a.group_size = 1;
    a.time = d_time;
    a.sun = d_sun;
    a.g_classes = d_classes;
    a.g_sky_raw = d_sky_raw;
    a.g_sky = d_sky;
    hipError_t e = ks ? launch_mlp_ks_group(m->W, a, m->n_cu, (hipStream_t)stream)
                : group_kernel_mode().load() == 0 ? launch_mlp_group_split(m->W, a, m->n_cu, (hipStream_t)stream)
                      : launch_mlp(PROG_GROUP, m->W, 0, false, a, m->n_cu, (hipStream_t)stream);      // bf16x3: its cost is 1/S of the field network's
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "group kernel launch");
}

static int field_launch(const snerf_model* m, int variant, MlpArgs& a, const snerf_field_out* out, void* stream) {
    // variant 3 (ray visibility) is reachable through snerf_field_ray_visibility only, which sets everything the RaySum epilogue dereferences
    if (variant < 0 || variant > 3 || (variant == 3 && !(a.out.vis && a.top && a.bot && a.tvals && !a.points)))
        return fail(SNERF_E_INVALID, "variant must be 0, 1 or 2 (3, ray visibility, only through snerf_field_ray_visibility)");
    if (variant == 3 && m->precision == SNERF_PREC_BF16) return fail(SNERF_E_INVALID, "ray visibility: not available in the bf16 fast mode");
    const FieldRoute r = field_route(m, variant);
    set_program(a, r);
    a.n_classes = m->C;
#ifdef SNERF_ABLATE
    if (const char* e = getenv("SNERF_ABLATE")) a.debug = (uint32_t)atoi(e);
#endif
    if (out) a.out = to_dev(out);      // (variant 3 comes without: its a.out.vis stays)
    if (variant <= 1 && !a.sun) return fail(SNERF_E_INVALID, "sun directions are required for variants 0 and 1");
    const hipStream_t st = (hipStream_t)stream;
    const hipError_t e = r.kernel == K_I8X2 ? launch_mlp_i8x2(m->W, variant, a, m->n_cu, st)
                       : r.kernel == K_I8   ? launch_mlp_i8(m->W, variant, a, m->n_cu, st)
                       : r.kernel == K_KS   ? launch_mlp_ks(m->W, variant, a, m->n_cu, st)
                                            : launch_mlp(PROG_FIELD, m->W, variant, m->precision == SNERF_PREC_BF16, a, m->n_cu, st);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "field kernel launch");
}

int snerf_field_forward_points(const snerf_model* m, int variant, int64_t n_points, const float* d_points,
                               int64_t group_size, const float* d_sun, const float* d_classes,
                               const snerf_field_out* out, void* stream) {
    int rc = check_ready(m);
    if (rc) return rc;
    if (n_points == 0) return SNERF_OK;
    if (n_points < 0 || !d_points || group_size < 1) return fail(SNERF_E_INVALID, "snerf_field_forward_points: bad argument");
    MlpArgs a = ray_args(m, n_points, nullptr, nullptr, nullptr, 1, group_size, 0);
    a.points = d_points;
    a.sun = d_sun;
    a.classes = d_classes;
    return field_launch(m, variant, a, out, stream);
}

int snerf_field_forward_rays(const snerf_model* m, int variant, int64_t n_rays, int n_samples, const float* d_top,
                             const float* d_bot, const float* d_tvals, int64_t rays_per_group, const float* d_sun,
                             const float* d_classes, const snerf_field_out* out, void* stream) {
    int rc = check_ready(m);
    if (rc) return rc;
    if (n_rays == 0) return SNERF_OK;
    if (n_rays < 0 || n_samples < 1 || rays_per_group < 1 || !d_top || !d_bot || !d_tvals)
        return fail(SNERF_E_INVALID, "snerf_field_forward_rays: bad argument");
    MlpArgs a = ray_args(m, n_rays * n_samples, d_top, d_bot, d_tvals, n_samples, (int64_t)n_samples * rays_per_group, 0);
    a.sun = d_sun;
    a.classes = d_classes;
    return field_launch(m, variant, a, out, stream);
}

int snerf_model_pack_sun_walk_host(snerf_model* m, int n_suns, uint8_t* stream_out, size_t* stream_bytes) {
    if (!m) return fail(SNERF_E_INVALID, "NULL model");
    if (n_suns < 1 || n_suns > kMaxWalkSuns) return fail(SNERF_E_INVALID, "snerf_model_pack_sun_walk_host: n_suns must be in [1," + std::to_string(kMaxWalkSuns) + "]");
    int rc = pack_both(m, true);
    if (rc) return rc;
    const bool ks = ks_width(m->W);
    const Packed& P = bf16_field(m).host;
    const int chunks = sun_walk_chunks(m->W, m->C, n_suns, ks);
    if (P.stream.size() != (size_t)field_chunk_start(m->W, m->C, F_NUM, ks) * kChunkBytes) return fail(SNERF_E_STATE, "snerf_model_pack_sun_walk_host: packed stream has an unexpected size");
    if (stream_bytes) *stream_bytes = (size_t)chunks * kChunkBytes;
    if (stream_out)
        for (int c = 0; c < chunks; ++c)
            std::memcpy(stream_out + (size_t)c * kChunkBytes, P.stream.data() + (size_t)sun_walk_source_chunk(m->W, m->C, n_suns, ks, c) * kChunkBytes, kChunkBytes);
    return SNERF_OK;
}

// device copy of the walk stream: whole layers' chunks out of the packed host stream, uploaded as snerf_model_finalize uploads the stream itself
// (synchronous copies: nothing here is stream-ordered, so nothing of it can end up in a captured graph)
static int walk_stream(const snerf_model* m, int n_suns) {
    if (m->d_walk && m->walk_suns == n_suns) return SNERF_OK;
    const bool ks = ks_width(m->W);
    const std::vector<uint8_t>& host = bf16_field(m).host.stream;
    const uint8_t* src = host.data();
    hipError_t e;
    if (m->d_walk) {                        // another n_suns: hipFree waits for the launches that still read the old copy
        if ((e = hipFree(m->d_walk)) != hipSuccess) return fail_hip(e, "hipFree");
        m->d_walk = nullptr;
        m->walk_suns = 0;
    }
    const size_t a = (size_t)field_chunk_start(m->W, m->C, F_S1, ks) * kChunkBytes, b = (size_t)field_chunk_start(m->W, m->C, F_A1, ks) * kChunkBytes,
                 end = (size_t)field_chunk_start(m->W, m->C, F_NUM, ks) * kChunkBytes;
    if (host.size() != end) return fail(SNERF_E_STATE, "sun walk: the packed field stream has an unexpected size");
    if ((e = hipMalloc((void**)&m->d_walk, (size_t)sun_walk_chunks(m->W, m->C, n_suns, ks) * kChunkBytes)) != hipSuccess) return fail_hip(e, "hipMalloc (walk stream)");
    e = hipMemcpy(m->d_walk, src, a, hipMemcpyHostToDevice);
    for (int j = 0; j < n_suns && e == hipSuccess; ++j) e = hipMemcpy(m->d_walk + a + (size_t)j * (b - a), src + a, b - a, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(m->d_walk + a + (size_t)n_suns * (b - a), src + b, end - b, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(m->d_walk);
        m->d_walk = nullptr;
        return fail_hip(e, "hipMemcpy (walk stream)");
    }
    m->walk_suns = n_suns;
    return SNERF_OK;
}

int snerf_field_sun_walk_rays(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                              int n_suns, const float* d_suns, const float* d_classes, const snerf_field_out* out, void* stream) {
    int rc = check_walk_model(m, "snerf_field_sun_walk_rays", "sun walk exists");
    if (rc) return rc;
    if (n_suns < 1 || n_suns > kMaxWalkSuns) return fail(SNERF_E_INVALID, "snerf_field_sun_walk_rays: n_suns must be in [1," + std::to_string(kMaxWalkSuns) + "]");
    if (n_rays < 0 || n_samples < 1 || !d_top || !d_bot || !d_tvals || !d_suns) return fail(SNERF_E_INVALID, "snerf_field_sun_walk_rays: bad argument");
    if (n_rays == 0) return SNERF_OK;
    rc = walk_stream(m, n_suns);
    if (rc) return rc;
    SunWalkArgs a{};
    a.n_suns = n_suns;
    a.m = ray_args(m, n_rays * n_samples, d_top, d_bot, d_tvals, n_samples, n_rays * n_samples, 0);
    set_program(a.m, bf16_field(m), (size_t)sun_walk_chunks(m->W, m->C, n_suns, ks_width(m->W)) * kChunkBytes);
    a.m.stream = m->d_walk;      // the walk stream in place of the program's own; the bias table is the program's
    a.m.sun = d_suns;
    a.m.classes = d_classes;
    if (out) a.m.out = to_dev(out);
    hipError_t e = launch_sun_walk(m->W, a, m->n_cu, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "sun walk kernel launch");
}

int snerf_field_ray_visibility(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot,
                               const float* d_tvals, int flags, float* d_vis, void* stream) {
    int rc = check_ready(m);
    if (rc) return rc;
    if (n_rays == 0) return SNERF_OK;
    if (n_rays < 0 || n_samples < 1 || !d_top || !d_bot || !d_tvals || !d_vis) return fail(SNERF_E_INVALID, "snerf_field_ray_visibility: bad argument");
    // variant 3: one ray per wave, ceil(S / 32) passes of 32 samples (kernels.h)
    MlpArgs a = ray_args(m, n_rays, d_top, d_bot, d_tvals, n_samples, 1,
                         (flags & 2) | (switches().rayvis_no_early_out ? 4 : 0) | (switches().rayvis_sun_first ? 8 : 0));
    a.out.vis = d_vis;
    return field_launch(m, 3, a, nullptr, stream);
}

int snerf_field_ray_surface(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                            int flags, float* d_out, void* stream) {
    if (n_rays < 0 || n_samples < 1 || !d_top || !d_bot || !d_tvals || !d_out || ((uintptr_t)d_out & 15))
        return fail(SNERF_E_INVALID, "snerf_field_ray_surface: bad argument (d_out must be 16-byte aligned)");
    int rc = check_walk_model(m, "snerf_field_ray_surface", "ray-surface kernels exist");
    if (rc) return rc;
    if (n_rays == 0) return SNERF_OK;
    RaySurfaceArgs a{};
    // one ray per wave (wave pair at width 512), ceil(S / 32) passes of 32 samples; bit 3: passes from t = 0 downwards, the order of the prefix
    a.m = ray_args(m, n_rays, d_top, d_bot, d_tvals, n_samples, 1, (flags & 6) | 8);
    set_program(a.m, field_route(m, 3));
    a.out = d_out;
    hipError_t e = launch_ray_surface(m->W, a, m->n_cu, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "ray surface kernel launch");
}

int snerf_field_shadow_walk(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_sun,
                            const float* d_tvals, int flags, float* d_out, void* stream) {
    if (n_rays < 0 || n_samples < 1 || !d_top || !d_bot || !d_sun || !d_tvals || !d_out || ((uintptr_t)d_out & 31))
        return fail(SNERF_E_INVALID, "snerf_field_shadow_walk: bad argument (d_out must be 32-byte aligned)");
    int rc = check_walk_model(m, "snerf_field_shadow_walk", "shadow-walk kernels exist");
    if (rc) return rc;
    if (n_rays == 0) return SNERF_OK;
    ShadowWalkArgs a{};
    // one ray per wave (wave pair at width 512), ceil(S / 32) passes of 32 samples, every one of them run; bit 3: passes from t = 0 downwards, the order of the prefix
    a.m = ray_args(m, n_rays, d_top, d_bot, d_tvals, n_samples, 1, (flags & 2) | 8);
    set_program(a.m, field_route(m, 1));
    a.sun = d_sun;
    a.out = d_out;
    hipError_t e = launch_shadow_walk(m->W, a, m->n_cu, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "shadow walk kernel launch");
}

int snerf_field_solar_audit(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                            const double* sun3, const float* d_est_vis, const float* d_ps, int flags, float* d_out, float* d_exact, void* stream) {
    if (n_rays < 0 || n_samples < 1 || !d_top || !d_bot || !d_tvals || !sun3 || !d_est_vis || !d_ps || !d_out || ((uintptr_t)d_out & 31))
        return fail(SNERF_E_INVALID, "snerf_field_solar_audit: bad argument (n_rays >= 0, n_samples >= 1, no NULL pointer but d_exact, d_out 32-byte aligned)");
    if (!std::isfinite(sun3[0]) || !std::isfinite(sun3[1]) || !std::isfinite(sun3[2]) || !(sun3[2] > 0.0) || !((float)sun3[2] > 0.f))
        return fail(SNERF_E_INVALID, "snerf_field_solar_audit: the sun direction must be finite with sun_z > 0");
    if (flags & ~6) return fail(SNERF_E_INVALID, "snerf_field_solar_audit: flags has bits other than 2 (outside the cube: delta 0) and 4 (no early-out)");
    if (!m) return fail(SNERF_E_INVALID, "snerf_field_solar_audit: NULL model");
    int rc = check_walk_model(m, "snerf_field_solar_audit", "solar-audit kernels exist");
    if (rc) return rc;
    if (n_rays == 0) return SNERF_OK;
    SolarAuditArgs a{};
    // primary rays: a workgroup walks the secondary rays of one ray's samples, four (width 512: two) at a time; bit 3 clear: passes from the point outwards
    a.m = ray_args(m, n_rays, d_top, d_bot, d_tvals, n_samples, 1, flags & 6);
    set_program(a.m, field_route(m, 3));
    for (int k = 0; k < 3; ++k) a.sun[k] = sun3[k];
    a.est_vis = d_est_vis;
    a.ps = d_ps;
    a.out = d_out;
    a.exact = d_exact;
    hipError_t e = launch_solar_audit(m->W, a, m->n_cu, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "solar audit kernel launch");
}

int snerf_field_frame_walk(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals, float delta,
                           const float* d_sun, const float* d_sky, int n_times, const float* d_class_vecs, int flags, float* d_out, void* stream) {
    if (n_rays < 0 || n_samples < 2 || !d_top || !d_bot || !d_tvals || !d_sun || !d_sky || !d_class_vecs || !d_out || ((uintptr_t)d_out & 63) ||
        n_times < 1 || n_times > kMaxFrameTimes || !std::isfinite(delta) || !(delta > 0.f))
        return fail(SNERF_E_INVALID, "snerf_field_frame_walk: bad argument (n_samples >= 2, n_times in [1," + std::to_string(kMaxFrameTimes) +
                                         "], delta finite and positive, d_out 64-byte aligned)");
    int rc = check_walk_model(m, "snerf_field_frame_walk", "frame-walk kernels exist");
    if (rc) return rc;
    if (n_rays == 0) return SNERF_OK;
    FrameWalkArgs a{};
    // one ray per wave (wave pair at width 512), ceil(S / 32) passes of 32 samples; bit 3: passes from t = 0 downwards, the order of the prefix
    a.m = ray_args(m, n_rays, d_top, d_bot, d_tvals, n_samples, 1, (flags & 6) | 8);
    set_program(a.m, field_route(m, 0));
    a.sun = d_sun;
    a.sky = d_sky;
    a.class_vecs = d_class_vecs;
    a.n_times = n_times;
    a.delta = delta;
    a.out = d_out;
    hipError_t e = launch_frame_walk(m->W, a, m->n_cu, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "frame walk kernel launch");
}

static int composite_rays(int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                          const float* d_rho, const float* d_col, const float* d_solar_vis, const float* d_sky,
                          int flags, const float* d_rho_prior, float trust, const float* d_trust, const snerf_composite_out* out, void* stream) {
    if (n_rays == 0) return SNERF_OK;
    if (n_rays < 0 || n_samples < 1 || !d_top || !d_bot || !d_tvals || !d_rho || !d_col || !d_solar_vis || !d_sky || !out)
        return fail(SNERF_E_INVALID, "snerf_composite_rays: bad argument");
    CompArgs a{};
    a.n_rays = n_rays; a.n_samples = n_samples;
    a.top = d_top; a.bot = d_bot; a.tvals = d_tvals;
    a.rho = d_rho; a.col = d_col; a.solar_vis = d_solar_vis; a.sky = d_sky;
    a.flags = flags; a.rho_prior = d_rho_prior; a.trust = trust; a.trust_dev = d_trust;
    a.out.rgb = out->d_rgb; a.out.albedo = out->d_albedo; a.out.pv = out->d_pv; a.out.pe = out->d_pe;
    a.out.ps = out->d_ps; a.out.delta = out->d_delta; a.out.shadow = out->d_shadow; a.out.acc = out->d_acc;
    a.out.surf_loc = out->d_surf_loc; a.out.surf_dist = out->d_surf_dist;
    hipError_t e = launch_composite(a, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "composite kernel launch");
}

int snerf_composite_rays(int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                         const float* d_rho, const float* d_col, const float* d_solar_vis, const float* d_sky,
                         int flags, const float* d_rho_prior, float trust, const snerf_composite_out* out, void* stream) {
    return composite_rays(n_rays, n_samples, d_top, d_bot, d_tvals, d_rho, d_col, d_solar_vis, d_sky, flags, d_rho_prior, trust, nullptr, out, stream);
}

int snerf_composite_rays_dt(int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                            const float* d_rho, const float* d_col, const float* d_solar_vis, const float* d_sky,
                            int flags, const float* d_rho_prior, const float* d_trust, const snerf_composite_out* out, void* stream) {
    if (d_rho_prior && !d_trust) return fail(SNERF_E_INVALID, "snerf_composite_rays_dt: d_trust is NULL");
    return composite_rays(n_rays, n_samples, d_top, d_bot, d_tvals, d_rho, d_col, d_solar_vis, d_sky, flags, d_rho_prior, 1.f, d_trust, out, stream);
}

// workspace layout of snerf_render_rays: classes [R,C] | sky_raw [R,3] | sky [R,3] | rho [N] | sv [N] | col [N,3]
static size_t align256(size_t x) { return (x + 255) / 256 * 256; }
size_t snerf_render_workspace_bytes(int64_t n_rays, int n_samples, int n_classes) {
    const size_t R = (size_t)n_rays, N = R * (size_t)n_samples;
    return align256(R * n_classes * 4) + 2 * align256(R * 3 * 4) + 2 * align256(N * 4) + align256(N * 3 * 4);
}

int snerf_render_rays(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot,
                      const float* d_tvals, const float* d_sun, const float* d_time, int flags, float* d_rgb,
                      const snerf_field_out* field_out, const snerf_composite_out* comp_out, void* d_workspace,
                      size_t workspace_bytes, void* stream) {
    int rc = check_ready(m);
    if (rc) return rc;
    if (n_rays == 0) return SNERF_OK;
    if (n_rays < 0 || n_samples < 1 || !d_top || !d_bot || !d_tvals || !d_sun || !d_time || !d_workspace)
        return fail(SNERF_E_INVALID, "snerf_render_rays: bad argument");
    if (workspace_bytes < snerf_render_workspace_bytes(n_rays, n_samples, m->C))
        return fail(SNERF_E_INVALID, "snerf_render_rays: workspace too small");
    const size_t R = (size_t)n_rays, N = R * (size_t)n_samples;
    char* ws = (char*)d_workspace;
    float* cls = (float*)ws; ws += align256(R * m->C * 4);
    float* sky_raw = (float*)ws; ws += align256(R * 3 * 4);
    float* sky = (float*)ws; ws += align256(R * 3 * 4);
    float* rho = (float*)ws; ws += align256(N * 4);
    float* sv = (float*)ws; ws += align256(N * 4);
    float* col = (float*)ws;
    rc = snerf_group_forward(m, n_rays, d_time, d_sun, cls, sky_raw, sky, stream);
    if (rc) return rc;
    snerf_field_out fo{};
    if (field_out) fo = *field_out;
    if (!fo.d_rho) fo.d_rho = rho;
    if (!fo.d_solar_vis) fo.d_solar_vis = sv;
    if (!fo.d_col) fo.d_col = col;
    rc = snerf_field_forward_rays(m, 0, n_rays, n_samples, d_top, d_bot, d_tvals, 1, d_sun, cls, &fo, stream);
    if (rc) return rc;
    snerf_composite_out co{};
    if (comp_out) co = *comp_out;
    if (d_rgb) co.d_rgb = d_rgb;
    return snerf_composite_rays(n_rays, n_samples, d_top, d_bot, d_tvals, fo.d_rho, fo.d_col, fo.d_solar_vis, sky, flags,
                                nullptr, 1.f, &co, stream);
}

int snerf_composite_sweep(int64_t n_rays, int n_samples, int n_classes, int n_times, const float* d_top,
                          const float* d_bot, const float* d_tvals, const float* d_deltas, const float* d_rho, const float* d_col_raw,
                          const float* d_adjust, const float* d_solar_vis, const float* d_sky, const float* d_class_vecs,
                          int flags, const snerf_sweep_out* out, void* stream) {
    if (n_rays == 0 || n_times == 0) return SNERF_OK;
    if (n_rays < 0 || n_samples < 1 || n_times < 0 || n_classes < 1 || n_classes > kMaxClasses ||
        (!d_deltas && (!d_top || !d_bot || !d_tvals)) || !d_rho || !d_col_raw || !d_adjust || !d_solar_vis || !d_sky || !d_class_vecs || !out)
        return fail(SNERF_E_INVALID, "snerf_composite_sweep: bad argument");
    SweepArgs a{};
    a.n_rays = n_rays; a.n_samples = n_samples; a.n_classes = n_classes; a.n_times = n_times; a.flags = flags;
    a.top = d_top; a.bot = d_bot; a.tvals = d_tvals; a.deltas = d_deltas; a.classic = out->d_classic;
    a.rho = d_rho; a.col_raw = d_col_raw; a.adjust = d_adjust;
    a.adjust_vec4 = (n_classes == 4 && (reinterpret_cast<uintptr_t>(d_adjust) & 15) == 0) ? 1 : 0;
    a.solar_vis = d_solar_vis; a.sky = d_sky; a.class_vecs = d_class_vecs;
    a.season = out->d_season; a.shaded = out->d_shaded; a.base = out->d_base; a.shadow_adjust = out->d_shadow_adjust;
    a.raw_shadow = out->d_raw_shadow;
    hipError_t e = launch_sweep(a, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "sweep kernel launch");
}

int snerf_composite_sun_walk(int64_t n_rays, int n_samples, int n_classes, int n_times, int n_suns, const float* d_top, const float* d_bot,
                             const float* d_tvals, const float* d_deltas, const float* d_rho, const float* d_col_raw, const float* d_adjust,
                             const float* d_solar_vis, const float* d_sky, const float* d_class_vecs, int flags, const snerf_sun_walk_out* out, void* stream) {
    if (n_rays < 0 || n_samples < 1 || n_times < 0 || n_suns < 0 || n_classes < 1 || n_classes > kMaxClasses || !out)
        return fail(SNERF_E_INVALID, "snerf_composite_sun_walk: bad argument");
    if (n_rays == 0 || (n_times == 0 && n_suns == 0)) return SNERF_OK;
    if ((!d_deltas && (!d_top || !d_bot || !d_tvals)) || !d_rho || !d_col_raw || !d_adjust || (n_suns && (!d_solar_vis || !d_sky)) || (n_times && !d_class_vecs))
        return fail(SNERF_E_INVALID, "snerf_composite_sun_walk: bad argument");
    if (sun_walk_composite_lds_bytes(n_samples, n_suns) > 64 * 1024)
        return fail(SNERF_E_INVALID, "snerf_composite_sun_walk: n_samples + 3 n_suns must not exceed 4096 (a ray's weights and shadow factors wait in LDS)");
    SunWalkCompArgs a{};
    a.n_rays = n_rays; a.n_samples = n_samples; a.n_classes = n_classes; a.n_times = n_times; a.n_suns = n_suns; a.flags = flags;
    a.top = d_top; a.bot = d_bot; a.tvals = d_tvals; a.deltas = d_deltas;
    a.rho = d_rho; a.col_raw = d_col_raw; a.adjust = d_adjust; a.solar_vis = d_solar_vis; a.sky = d_sky; a.class_vecs = d_class_vecs;
    a.shaded = out->d_shaded; a.season = out->d_season; a.base = out->d_base; a.raw_shadow = out->d_raw_shadow; a.shadow_adjust = out->d_shadow_adjust;
    hipError_t e = launch_sun_walk_composite(a, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "sun walk compositing kernel launch");
}

int snerf_rays_from_camera(const double* P_3x4, int rows, int cols, int downscale, float* d_rows, uint8_t* d_valid, void* stream) {
    if (!P_3x4 || rows < 0 || cols < 0 || downscale < 1 || !d_rows) return fail(SNERF_E_INVALID, "snerf_rays_from_camera: bad argument");
    RayGenArgs a{};
    for (int i = 0; i < 12; ++i) a.P[i] = P_3x4[i];
    a.rows = rows; a.cols = cols; a.ds = downscale; a.rows_out = d_rows; a.valid = d_valid;
    hipError_t e = launch_rays_from_camera(a, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "ray generation kernel launch");
}

int snerf_ray_grid(int mode, int rows, int cols, int64_t lo, int64_t hi, const double* params, int n_params, float* d_top, float* d_bot, uint8_t* d_valid,
                   int32_t* d_pixels, void* stream) {
    if (mode < 0 || mode > 2 || rows < 1 || cols < 1 || lo < 0 || hi < lo || hi > (int64_t)rows * cols || !params || (hi > lo && (!d_top || !d_bot)))
        return fail(SNERF_E_INVALID, "snerf_ray_grid: bad argument");
    RayGridArgs a{};
    a.mode = mode; a.rows = rows; a.cols = cols; a.lo = lo; a.hi = hi; a.top = d_top; a.bot = d_bot; a.valid = d_valid; a.pix = d_pixels;
    if (mode == 2) {
        if (n_params != 14 || params[12] < 1 || params[13] < 1) return fail(SNERF_E_INVALID, "snerf_ray_grid: mode 2 takes the 12 camera entries + image rows, cols");
        for (int i = 0; i < 12; ++i) a.P[i] = params[i];
        a.img_rows = (int)params[12]; a.img_cols = (int)params[13];
    } else {
        if (n_params != 3 && !(mode == 1 && n_params == 7)) return fail(SNERF_E_INVALID, "snerf_ray_grid: modes 0 / 1 take the view vector / v_z (3 doubles) [+ region (4)]");
        for (int i = 0; i < 3; ++i) a.q[i] = params[i];
        a.has_region = n_params == 7;
        for (int i = 0; i < 4 && a.has_region; ++i) a.region[i] = params[3 + i];
    }
    hipError_t e = launch_ray_grid(a, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "ray grid kernel launch");
}

int snerf_prior_density(int64_t n_points, const float* d_points, const float* d_delta, const double* d_height_map, int hm_rows, int hm_cols,
                        const float* d_outside, float* d_rho_prior, void* stream) {
    if (n_points < 0) return fail(SNERF_E_INVALID, "snerf_prior_density: negative point count");
    if (n_points == 0) return SNERF_OK;
    if (!d_points || !d_delta || !d_height_map || !d_rho_prior || hm_rows < 1 || hm_cols < 1)
        return fail(SNERF_E_INVALID, "snerf_prior_density: bad argument");
    const float term = -logf(1.0f - 0.99f);          // Prob_exist clamped to .99 (T_NeRF_net_v2.py:178-179)
    hipError_t e = launch_prior_density(n_points, d_points, d_delta, d_height_map, hm_rows, hm_cols, d_outside, term, d_rho_prior,
                                        (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "prior density kernel launch");
}

int snerf_surface_distance(int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                           const double* d_dsm, int dsm_rows, int dsm_cols, const double* d_levels, double* d_dist, void* stream) {
    if (n_rays < 0 || n_samples < 1) return fail(SNERF_E_INVALID, "snerf_surface_distance: bad ray/sample count");
    if (n_rays == 0) return SNERF_OK;
    if (!d_top || !d_bot || !d_tvals || !d_dsm || !d_levels || !d_dist || dsm_rows < 1 || dsm_cols < 1)
        return fail(SNERF_E_INVALID, "snerf_surface_distance: bad argument");
    hipError_t e = launch_surface_distance(n_rays, n_samples, d_top, d_bot, d_tvals, d_dsm, dsm_rows, dsm_cols, d_levels, d_dist,
                                           (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "surface distance kernel launch");
}

int snerf_image_error(int64_t n_pixels, const float* d_image, const float* d_gt, double* d_sums, void* stream) {
    if (n_pixels < 0) return fail(SNERF_E_INVALID, "snerf_image_error: negative pixel count");
    if (n_pixels == 0) return SNERF_OK;
    if (!d_image || !d_gt || !d_sums) return fail(SNERF_E_INVALID, "snerf_image_error: bad argument");
    hipError_t e = launch_image_error(n_pixels, d_image, d_gt, d_sums, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "image error kernel launch");
}

int snerf_transmittance(int64_t n_rays, int n_samples, const float* d_rho, const float* d_delta, float* d_pv, void* stream) {
    if (n_rays < 0 || n_samples < 0) return fail(SNERF_E_INVALID, "snerf_transmittance: negative size");
    if (n_rays == 0 || n_samples == 0) return SNERF_OK;
    if (!d_rho || !d_delta || !d_pv) return fail(SNERF_E_INVALID, "snerf_transmittance: bad argument");
    hipError_t e = launch_transmittance(n_rays, n_samples, d_rho, d_delta, d_pv, (hipStream_t)stream);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "transmittance kernel launch");
}

int snerf_field_kernel_info(const snerf_model* m, int64_t n_points, int* grid, int* block, int* lds_bytes) {
    if (!m) return fail(SNERF_E_INVALID, "NULL model");
    int rc = pack_both(const_cast<snerf_model*>(m));
    if (rc) return rc;
    const FieldRoute r = field_route(m, 0);      // what field_launch launches for variant 0
    const int64_t tiles = (n_points + r.tile_points - 1) / r.tile_points;
    const int ncu = m->n_cu ? m->n_cu : 256;
    if (grid) *grid = (int)(tiles < ncu ? tiles : ncu);
    if (block) *block = r.block;
    if (lds_bytes) *lds_bytes = r.lds_bytes;
    return SNERF_OK;
}

// ---- device ray loader (csrc/loader.hip; arithmetic shared with the host mirrors: csrc/loader_common.h)
static int64_t loader_batches_per_epoch(int64_t n, int64_t batch, int drop_last, int world) {
    return drop_last ? n / (batch * world) : (n + batch - 1) / batch;
}
static void loader_advance_host(int64_t* s, int64_t bpe) {      // the rule of loader_advance_kernel
    s[2] += 1;
    if (++s[1] >= bpe) { s[1] = 0; s[0] += 1; }
}
static void loader_bounds(const float* bounds6, float* b) {     // SC_loader.__init__: x = bounds[0,0], dx = bounds[0,1] - bounds[0,0] (fp32), ...
    static const float cube[6] = {-1.f, 1.f, -1.f, 1.f, -1.f, 1.f};
    const float* s = bounds6 ? bounds6 : cube;
    b[0] = s[0]; b[1] = s[1] - s[0]; b[2] = s[2]; b[3] = s[3] - s[2]; b[4] = s[4]; b[5] = s[5];
}
static bool stream_capturing(void* stream) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing((hipStream_t)stream, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return cs != hipStreamCaptureStatusNone;
}

int snerf_loader_create(const float* d_table, int64_t n_rows, int row_width, int64_t batch, uint64_t seed, int drop_last, int rank, int world,
                        const float* bounds6, snerf_loader** out) {
    if (!out) return fail(SNERF_E_INVALID, "snerf_loader_create: NULL result pointer");
    *out = nullptr;
    if (!d_table) return fail(SNERF_E_INVALID, "snerf_loader_create: NULL table");
    if (row_width != kLoaderCols) return fail(SNERF_E_INVALID, "snerf_loader_create: the ray table has 22 columns, got " + std::to_string(row_width));
    if (n_rows < 1) return fail(SNERF_E_INVALID, "snerf_loader_create: n_rows < 1");
    if (batch < 1 || batch > 0x7fffffffLL) return fail(SNERF_E_INVALID, "snerf_loader_create: batch must be in [1, 2^31)");
    if (world < 1 || rank < 0 || rank >= world) return fail(SNERF_E_INVALID, "snerf_loader_create: rank outside [0, world)");
    if (world > 1 && !drop_last) return fail(SNERF_E_INVALID, "snerf_loader_create: world > 1 needs drop_last (every rank must see the same number of full batches)");
    if (drop_last && batch * world > n_rows) return fail(SNERF_E_INVALID, "snerf_loader_create: batch * world > n_rows with drop_last - an epoch would be empty");
    snerf_loader* l = new snerf_loader();
    l->d_table = d_table; l->n = n_rows; l->batch = batch; l->seed = seed; l->drop_last = drop_last ? 1 : 0; l->rank = rank; l->world = world;
    l->bits = loader_bits(n_rows);
    l->bpe = loader_batches_per_epoch(n_rows, batch, l->drop_last, world);
    loader_bounds(bounds6, l->b);
    hipError_t e = hipMalloc((void**)&l->d_state, 4 * sizeof(int64_t));
    if (e == hipSuccess) e = hipMemcpy(l->d_state, l->shadow, 4 * sizeof(int64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        if (l->d_state) (void)hipFree(l->d_state);
        delete l;
        return fail_hip(e, "snerf_loader_create: state allocation");
    }
    *out = l;
    return SNERF_OK;
}

void snerf_loader_destroy(snerf_loader* l) {
    if (!l) return;
    if (l->d_state) (void)hipFree(l->d_state);
    delete l;
}

int64_t snerf_loader_batches_per_epoch(const snerf_loader* l) {
    if (!l) return fail(SNERF_E_INVALID, "NULL loader");
    return l->bpe;
}

int64_t snerf_loader_batch(const snerf_loader* l) {
    if (!l) return fail(SNERF_E_INVALID, "NULL loader");
    return l->batch;
}

int64_t snerf_loader_next(snerf_loader* l, const snerf_loader_out* out, void* stream) {
    if (!l || !out) return fail(SNERF_E_INVALID, "snerf_loader_next: NULL loader or outputs");
    const bool uniform = l->bpe * l->batch * l->world <= l->n && (l->drop_last || l->n % l->batch == 0);
    const bool capturing = stream_capturing(stream);
    if (capturing && !uniform)
        return fail(SNERF_E_STATE, "snerf_loader_next: a captured draw replays with a fixed row count - the epoch's last batch is short (use drop_last)");
    const int64_t p0 = (l->shadow[1] * l->world + l->rank) * l->batch;
    const int64_t rows = uniform ? l->batch : (l->n - p0 < l->batch ? l->n - p0 : l->batch);
    if (rows < 1) return fail(SNERF_E_STATE, "snerf_loader_next: the host shadow of the position is past the epoch's end");
    LoaderArgs a{};
    a.table = l->d_table; a.n_rows = l->n; a.batch = l->batch; a.rows = rows; a.batches_per_epoch = l->bpe; a.state = l->d_state; a.seed = l->seed;
    a.rank = l->rank; a.world = l->world; a.bits = l->bits;
    a.img_pt = out->d_img_pt; a.top = out->d_top; a.bot = out->d_bot; a.view = out->d_view_angle; a.sun = out->d_sun_angle; a.time = out->d_time_encoded;
    a.weight = out->d_sample_weight; a.gt = out->d_gt_color; a.index = out->d_row_index; a.sc_top = out->d_sc_top; a.sc_bot = out->d_sc_bot;
    a.x0 = l->b[0]; a.dx = l->b[1]; a.y0 = l->b[2]; a.dy = l->b[3]; a.z_lo = l->b[4]; a.z_hi = l->b[5];
    hipError_t e = launch_loader_draw(a, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "loader draw kernel launch");
    e = launch_loader_advance(l->d_state, l->bpe, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "loader advance kernel launch");
    if (!capturing) loader_advance_host(l->shadow, l->bpe);      // (a capture executes nothing; its replays advance the device copy only)
    return rows;
}

int snerf_loader_get_state(snerf_loader* l, int64_t* state4, void* stream) {
    if (!l || !state4) return fail(SNERF_E_INVALID, "snerf_loader_get_state: NULL argument");
    if (stream_capturing(stream)) return fail(SNERF_E_STATE, "snerf_loader_get_state: the stream is capturing");
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);      // the draws queued so far have advanced the state; then a blocking copy (never a stream-ordered
    if (e == hipSuccess) e = hipMemcpy(state4, l->d_state, 4 * sizeof(int64_t), hipMemcpyDeviceToHost);      // runtime copy in this library: DESIGN 5.4c)
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "snerf_loader_get_state");
}

int snerf_loader_set_state(snerf_loader* l, const int64_t* state4, void* stream) {
    if (!l || !state4) return fail(SNERF_E_INVALID, "snerf_loader_set_state: NULL argument");
    if (state4[0] < 0 || state4[1] < 0 || state4[1] >= l->bpe || state4[2] < 0)
        return fail(SNERF_E_INVALID, "snerf_loader_set_state: epoch / draws negative or batch_in_epoch outside [0, batches per epoch)");
    if (stream_capturing(stream)) return fail(SNERF_E_STATE, "snerf_loader_set_state: the stream is capturing");
    for (int i = 0; i < 4; ++i) l->shadow[i] = state4[i];
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);      // no draw in flight reads the state while the blocking copy replaces it
    if (e == hipSuccess) e = hipMemcpy(l->d_state, l->shadow, 4 * sizeof(int64_t), hipMemcpyHostToDevice);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "snerf_loader_set_state");
}

int snerf_loader_indices_host(int64_t n_rows, uint64_t seed, int64_t epoch, int64_t first, int64_t count, int64_t* out) {
    if (n_rows < 1 || epoch < 0 || first < 0 || count < 0 || first > n_rows - count || (count > 0 && !out))
        return fail(SNERF_E_INVALID, "snerf_loader_indices_host: need n_rows >= 1, epoch >= 0 and [first, first + count) inside [0, n_rows)");
    const int bits = loader_bits(n_rows);
    const LoaderKeys K = loader_keys(seed, (uint64_t)epoch);
    for (int64_t j = 0; j < count; ++j) out[j] = loader_perm(first + j, n_rows, bits, K);
    return SNERF_OK;
}

int snerf_loader_sc_rays_host(uint64_t seed, int64_t draws, int rank, int64_t first, int64_t count, const float* bounds6, float* top, float* bot) {
    if (first < 0 || count < 0 || (count > 0 && (!top || !bot))) return fail(SNERF_E_INVALID, "snerf_loader_sc_rays_host: bad argument");
    float b[6];
    loader_bounds(bounds6, b);
    for (int64_t j = 0; j < count; ++j) {
        uint32_t w[4];
        loader_sc_words(seed, (uint64_t)draws, (uint32_t)rank, (uint32_t)(first + j), w);
        float u[4], v[4];
        for (int q = 0; q < 4; ++q) u[q] = loader_uniform(w[q]);
        for (int q = 0; q < 4; ++q) {
            const float prod = u[q] * ((q & 1) ? b[3] : b[1]);    // two roundings (this file is built with -ffp-contract=off), as __fmul_rn / __fadd_rn in the kernel
            v[q] = prod + ((q & 1) ? b[2] : b[0]);
        }
        top[j * 3] = v[0]; top[j * 3 + 1] = v[1]; top[j * 3 + 2] = b[5];
        bot[j * 3] = v[2]; bot[j * 3 + 1] = v[3]; bot[j * 3 + 2] = b[4];
    }
    return SNERF_OK;
}

int snerf_loader_philox_host(const uint32_t* counter4, const uint32_t* key2, uint32_t* out4) {
    if (!counter4 || !key2 || !out4) return fail(SNERF_E_INVALID, "snerf_loader_philox_host: NULL argument");
    philox4x32_10(counter4, key2, out4);
    return SNERF_OK;
}

// ---- per-step training inputs (csrc/loader.hip: step_inputs_draw_kernel; word assignment: csrc/loader_common.h)
// The device copy of the state is allocated by the first call that needs it (a draw, or get / set once a draw has run): creating a handle and moving its
// position touch no GPU, so a checkpoint can be prepared - and the argument checks tested - on a host without one.
static int step_inputs_device(snerf_step_inputs* h) {
    if (h->d_state) return SNERF_OK;
    hipError_t e = hipMalloc((void**)&h->d_state, 4 * sizeof(int64_t));
    if (e == hipSuccess) e = hipMemcpy(h->d_state, h->shadow, 4 * sizeof(int64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) return SNERF_OK;
    if (h->d_state) (void)hipFree(h->d_state);
    h->d_state = nullptr;
    return fail_hip(e, "snerf_step_inputs: state allocation");
}

int snerf_step_inputs_create(uint64_t seed, int64_t n_rays, int64_t n_samples, int rank, const double* W2L_H, const double* world_center,
                             const float* d_table, int64_t n_table_rows, snerf_step_inputs** out) {
    if (!out) return fail(SNERF_E_INVALID, "snerf_step_inputs_create: NULL result pointer");
    *out = nullptr;
    if (!W2L_H || !world_center || !d_table) return fail(SNERF_E_INVALID, "snerf_step_inputs_create: NULL matrix, centre or table");
    if (n_rays < 1 || n_rays > 0x7fffffffLL || n_samples < 1 || n_samples > 0x7fffffffLL)
        return fail(SNERF_E_INVALID, "snerf_step_inputs_create: n_rays and n_samples must be in [1, 2^31)");
    if (rank < 0 || (uint32_t)rank >= kStepInputsMaxRank) return fail(SNERF_E_INVALID, "snerf_step_inputs_create: rank outside [0, 2^24)");
    for (int i = 0; i < 16; ++i)
        if (!std::isfinite(W2L_H[i])) return fail(SNERF_E_INVALID, "snerf_step_inputs_create: non-finite matrix");
    for (int i = 0; i < 3; ++i)
        if (!std::isfinite(world_center[i])) return fail(SNERF_E_INVALID, "snerf_step_inputs_create: non-finite world centre");
    if (n_table_rows < 1) return fail(SNERF_E_INVALID, "snerf_step_inputs_create: n_table_rows < 1");
    snerf_step_inputs* h = new snerf_step_inputs();
    h->seed = seed; h->n_rays = n_rays; h->n_samples = n_samples; h->rank = rank; h->d_table = d_table; h->table_rows = n_table_rows;
    for (int i = 0; i < 12; ++i) h->H[i] = W2L_H[i];
    for (int i = 0; i < 3; ++i) h->wc[i] = world_center[i];
    h->lon_scale = 1000.0 * 6378.137 * std::cos(world_center[0] * (3.14159265358979323846 / 180.0));      // this file is built with -ffp-contract=off
    *out = h;
    return SNERF_OK;
}

void snerf_step_inputs_destroy(snerf_step_inputs* h) {
    if (!h) return;
    if (h->d_state) (void)hipFree(h->d_state);
    delete h;
}

int64_t snerf_step_inputs_rays(const snerf_step_inputs* h) { return h ? h->n_rays : fail(SNERF_E_INVALID, "NULL step-inputs handle"); }
int64_t snerf_step_inputs_samples(const snerf_step_inputs* h) { return h ? h->n_samples : fail(SNERF_E_INVALID, "NULL step-inputs handle"); }
int64_t snerf_step_inputs_table_rows(const snerf_step_inputs* h) { return h ? h->table_rows : fail(SNERF_E_INVALID, "NULL step-inputs handle"); }

int snerf_step_inputs_draw(snerf_step_inputs* h, const snerf_step_inputs_out* out, void* stream) {
    if (!h || !out) return fail(SNERF_E_INVALID, "snerf_step_inputs_draw: NULL handle or outputs");
    if ((out->d_tv_image || out->d_tv_solar) && !out->d_base) return fail(SNERF_E_INVALID, "snerf_step_inputs_draw: the jitter outputs need d_base");
    const bool capturing = stream_capturing(stream);
    if (capturing && !h->d_state) return fail(SNERF_E_STATE, "snerf_step_inputs_draw: the first draw of a handle allocates its state - draw once before capturing");
    if (int rc = step_inputs_device(h)) return rc;
    StepInputsArgs a{};
    a.state = h->d_state; a.seed = h->seed; a.rank = (uint32_t)h->rank; a.n_rays = h->n_rays; a.n_samples = h->n_samples;
    for (int i = 0; i < 12; ++i) a.H[i] = h->H[i];
    for (int i = 0; i < 3; ++i) a.wc[i] = h->wc[i];
    a.lon_scale = h->lon_scale;
    a.inv_s = (float)(1.0 / (double)h->n_samples);
    a.base = out->d_base; a.table = h->d_table; a.table_rows = h->table_rows;
    a.starts = out->d_starts; a.ends = out->d_ends; a.vec = out->d_vec; a.times = out->d_times; a.tv_image = out->d_tv_image; a.tv_solar = out->d_tv_solar;
    a.hyper = out->d_hyper; a.trust = out->d_trust; a.lr2 = out->d_lr2;
    hipError_t e = launch_step_inputs_draw(a, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "step inputs draw kernel launch");
    e = launch_step_inputs_advance(h->d_state, (hipStream_t)stream);
    if (e != hipSuccess) return fail_hip(e, "step inputs advance kernel launch");
    if (!capturing) { h->shadow[0] += 1; h->shadow[1] += 1; }      // (a capture executes nothing; its replays advance the device copy only)
    return SNERF_OK;
}

int snerf_step_inputs_get_state(snerf_step_inputs* h, int64_t* state4, void* stream) {
    if (!h || !state4) return fail(SNERF_E_INVALID, "snerf_step_inputs_get_state: NULL argument");
    if (!h->d_state) {                                             // nothing has run on the device yet: the shadow is the state
        for (int i = 0; i < 4; ++i) state4[i] = h->shadow[i];
        return SNERF_OK;
    }
    if (stream_capturing(stream)) return fail(SNERF_E_STATE, "snerf_step_inputs_get_state: the stream is capturing");
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);
    if (e == hipSuccess) e = hipMemcpy(state4, h->d_state, 4 * sizeof(int64_t), hipMemcpyDeviceToHost);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "snerf_step_inputs_get_state");
}

int snerf_step_inputs_set_state(snerf_step_inputs* h, const int64_t* state4, void* stream) {
    if (!h || !state4) return fail(SNERF_E_INVALID, "snerf_step_inputs_set_state: NULL argument");
    if (state4[0] < 0 || state4[1] < 0) return fail(SNERF_E_INVALID, "snerf_step_inputs_set_state: draws or step negative");
    if (h->d_state && stream_capturing(stream)) return fail(SNERF_E_STATE, "snerf_step_inputs_set_state: the stream is capturing");
    for (int i = 0; i < 4; ++i) h->shadow[i] = state4[i];
    if (!h->d_state) return SNERF_OK;                              // the device copy starts from the shadow when the first draw creates it
    hipError_t e = hipStreamSynchronize((hipStream_t)stream);      // no draw in flight reads the state while the blocking copy replaces it
    if (e == hipSuccess) e = hipMemcpy(h->d_state, h->shadow, 4 * sizeof(int64_t), hipMemcpyHostToDevice);
    return e == hipSuccess ? SNERF_OK : fail_hip(e, "snerf_step_inputs_set_state");
}

int snerf_step_inputs_words_host(uint64_t seed, int64_t draws, int rank, int64_t n_rays, int64_t n_samples, uint32_t* ray_words, uint32_t* sample_words) {
    if (draws < 0 || rank < 0 || (uint32_t)rank >= kStepInputsMaxRank || n_rays < 0 || n_rays > 0x7fffffffLL || n_samples < 0 || n_samples > 0x7fffffffLL ||
        (n_rays > 0 && !ray_words) || (n_samples > 0 && !sample_words))
        return fail(SNERF_E_INVALID, "snerf_step_inputs_words_host: bad argument");
    for (int64_t i = 0; i < n_rays; ++i) {
        step_inputs_words(seed, (uint64_t)draws, (uint32_t)rank, 0, (uint32_t)i, ray_words + i * 8);
        step_inputs_words(seed, (uint64_t)draws, (uint32_t)rank, 1, (uint32_t)i, ray_words + i * 8 + 4);
    }
    for (int64_t s = 0; s < n_samples; ++s) step_inputs_words(seed, (uint64_t)draws, (uint32_t)rank, 2, (uint32_t)s, sample_words + s * 4);
    return SNERF_OK;
}

}  // extern "C"
