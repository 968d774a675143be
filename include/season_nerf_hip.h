/* season_nerf_hip.h - C ABI of the MI355X-native Season-NeRF per-ray hot path.
 *
 * The reference (EnterpriseCV-6/Season-NeRF) is pure PyTorch and has no FFI; its seams are Python call
 * signatures.  This library sits UNDER those seams: every entry point below names the reference
 * function(s) whose device work it replaces.  Plain pointers and sizes only - no torch types.
 *
 * Conventions
 *   - every `d_*` pointer is DEVICE memory (HBM) owned by the caller; fp32, contiguous, row-major;
 *     NULL for an optional output means "do not produce it";
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); all work is asynchronous on it;
 *   - functions return 0 on success, a negative SNERF_E_* code on failure and never throw;
 *     snerf_last_error() returns a thread-local description of the last failure;
 *   - a model is immutable after snerf_model_finalize(); one model may be used from several streams.
 */
#ifndef SEASON_NERF_HIP_H
#define SEASON_NERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SNERF_OK 0
#define SNERF_E_INVALID (-1)   /* bad argument (shape, width, NULL where required) */
#define SNERF_E_MISSING (-2)   /* a required state_dict tensor was not set */
#define SNERF_E_HIP (-3)       /* HIP runtime error (no device, launch failure, ...) */
#define SNERF_E_STATE (-4)     /* call order error (e.g. forward before finalize) */

typedef struct snerf_model snerf_model;

const char* snerf_last_error(void);
/* ABI version of this header; bumped on any signature change. */
int snerf_abi_version(void);

/* ---- model: the reference's T_NeRF(layer_width, n_classes) state_dict  (T_NeRF_net_v2.py:20-60)
 * snerf_model_set_tensor takes the checkpoint keys unchanged ("G_NeRF_net.fc2.linear.weight",
 * "G_NeRF_net.fc2.norm.running_var", "adjust_col.bias", ...): HOST fp32 data, numel elements.
 * Unknown keys (the dead heads adjust_rho/adjust_solar_vis/adjust_sky_col, num_batches_tracked) are accepted and
 * ignored.  snerf_model_finalize folds eval-mode BatchNorm (misc.py:169-170), packs the MFMA fragment streams on
 * the host and uploads them (the only call of this group that touches the GPU). */
snerf_model* snerf_model_create(int layer_width, int n_classes);
int snerf_model_set_tensor(snerf_model* m, const char* key, const float* host_data, size_t numel);
int snerf_model_finalize(snerf_model* m);
void snerf_model_destroy(snerf_model* m);
int snerf_model_width(const snerf_model* m);
int snerf_model_classes(const snerf_model* m);

/* Arithmetic of the fused per-point (field) network; set before snerf_model_finalize.  The reference computes in fp32
 * (plain torch, T_NeRF_net_v2.py:75-105); the north-star bar is 1e-4 relative on RGB / depth against it.
 *   SNERF_PREC_BF16X3  3-term error-compensated bf16 MFMA products, fp32 accumulate: RGB ~3e-6, per-sample outputs ~1e-5 (C-ABI default);
 *                      widths 64 / 256: one wave per 32 points (csrc/kernels.hip); width 512, the reference's default (main_lite.py:80):
 *                      every layer's K split over a pair of waves (csrc/kernels_ks.hip)
 *   SNERF_PREC_BF16    one bf16 MFMA per product (first layer keeps 3 terms): RGB 2-3e-3 - outside the bar, "fast" mode (widths 64 / 256)
 *   SNERF_PREC_I8X3    16-bit fixed point in two int8 digits on the int8 MFMA pipe, exact integer accumulation:
 *                      RGB ~2e-5, per-sample outputs ~1e-4; any input range (the raw coordinates of the encodings enter in fp32)
 *   SNERF_PREC_AUTO    SNERF_PREC_I8X3 where the packed weights clear its pack-time error bound (snerf_model_i8_estimate),
 *                      SNERF_PREC_BF16X3 otherwise; resolved when the weights are packed (snerf_model_resolve_precision or
 *                      snerf_model_finalize), after which snerf_model_precision reports the mode chosen
 * The per-group network (class softmax, sky colour: one row per ray, its error is not averaged over a ray's samples) runs in
 * BF16X3 at every width, whatever the mode (512: on the wave-pair structure of csrc/kernels_ks.hip; exact fp32 layer by layer in rounds 3-5). */
#define SNERF_PREC_BF16X3 0
#define SNERF_PREC_BF16 1
#define SNERF_PREC_I8X3 2
#define SNERF_PREC_AUTO 3
int snerf_model_set_precision(snerf_model* m, int precision);
int snerf_model_precision(const snerf_model* m);

/* What SNERF_PREC_I8X3 would add to the network's outputs for THESE weights, predicted on the host from the packed integers
 * (no GPU): per output row the rounding of its weights to 16 bits of the row maximum, of the activations to 16 bits of
 * [-1, 1] and the dropped low x low digit product, carried through the layers (a sine layer multiplies an error by
 * 2 pi |cos|).  `*_rms` are absolute RMS errors of the raw (pre-softplus / pre-sigmoid) head outputs; the reference's
 * fp32 arithmetic (T_NeRF_net_v2.py:75-105) is the zero point.  `rgb_pred` weighs them by what each head moves in the rendered
 * colour and depth (Eval_Tools_2.py:187-215): the predicted worst relative error over a batch of rays, about twice what is
 * observed (calibrated on weight sets with heavy tails, outliers and high gains, against fp64 and - tests/golden/stress_*.npz -
 * against the reference itself); `budget` is the value it must stay under (the north star's 1e-4).  `acc_bound` is the exact
 * maximum of the int32 accumulator expression (M << 8) + X over all rows and all possible activations.
 * ok = rgb_pred <= budget && acc_bound < 2^31.  Works before or after snerf_model_finalize, under any precision setting. */
typedef struct snerf_i8_estimate {
    double head_rms[4];   /* density, colour, solar visibility, seasonal adjust */
    double hidden_rms;    /* worst hidden layer: RMS error of its activations */
    double worst;         /* max over head_rms */
    double rgb_pred;
    double budget;
    int64_t acc_bound;
    int ok;
} snerf_i8_estimate;
int snerf_model_i8_estimate(snerf_model* m, snerf_i8_estimate* out);
/* Packs on the host if that has not happened yet and returns the precision the model runs in (SNERF_PREC_AUTO resolved),
 * or a negative SNERF_E_* code (SNERF_E_INVALID: the mode asked for has no kernel at this width - SNERF_PREC_BF16 at 512). */
int snerf_model_resolve_precision(snerf_model* m);

/* Host-only packing (no GPU): sizes and bytes of the packed programs, for tests and offline tooling.
 * program 0 = per-point field network, 1 = per-group (time/sun) network (bf16 hi/lo fragment pairs + bias table);
 * program 2 = the field network in the int8-digit format (T/L digit fragment pairs + per-row [scale | bias] tables),
 * only under SNERF_PREC_I8X3; program 3 = the field network's bf16 pairs in the K-split order of the width-512 kernel
 * (csrc/program.h ks_*: a permutation of program 0's pairs, same bias table), program 4 = program 1's pairs in that order; 3 and 4: width 512 only;
 * program 5 = program 2's digits in the layout of the 16x16x64 int8 matrix instruction (csrc/program.h k64_*), only under SNERF_PREC_I8X3 at width 256.
 * Buffers may be NULL to query sizes. */
int snerf_model_pack_host(snerf_model* m, int program, uint8_t* stream_out, size_t* stream_bytes,
                          float* bias_out, size_t* bias_floats);

/* ---- per-group network: T_NeRF.get_class_only (T_NeRF_net_v2.py:160-163) and the sky-colour head
 * (G_NeRF.py:110-111).  time is [G,4] (columns 0:2 are used, T_NeRF_net_v2.py:72-73), sun is [G,3].
 * Outputs: classes [G,C] softmax, sky_raw [G,3] pre-sigmoid, sky [G,3] sigmoid. */
int snerf_group_forward(const snerf_model* m, int64_t n_groups, const float* d_time, const float* d_sun,
                        float* d_classes, float* d_sky_raw, float* d_sky, void* stream);
/* Which kernel snerf_group_forward launches at widths 64 and 256, process-wide: 0 = one 32-ray tile per workgroup with every layer's
 * output blocks split over the four waves (csrc/kernels_group.hip; the default), 1 = one wave per 32 rays (csrc/kernels.hip).  The two
 * give bit-identical outputs; 1 exists for A/B timing and as the reference of the bit-identity test.  SNERF_GROUP_ONE_WAVE in the
 * environment (read once) makes 1 the initial value.  Width 512 has one kernel and ignores the mode. */
int snerf_set_group_kernel(int mode);

/* ---- per-point field network on explicit points: device part of T_NeRF.forward / forward_seperate /
 * forward_full_eval / forward_Solar / forward_Classic_Sigma_Only (T_NeRF_net_v2.py:75-204).
 * Point n uses sun/classes row n / group_size.  variant: 0 = everything, 1 = density + solar visibility only
 * (forward_Solar), 2 = density only (forward_Classic_Sigma_Only).
 * Outputs (all optional): rho [N] softplus, solar_vis [N] sigmoid, col_raw [N,3], adjust [N,C,3],
 * col [N,3] = sigmoid(col_raw + sum_c classes_c * adjust_c), adjust_col [N,3]. */
typedef struct snerf_field_out {
    float* d_rho;
    float* d_solar_vis;
    float* d_col_raw;
    float* d_adjust;
    float* d_col;
    float* d_adjust_col;
    float* d_points;      /* [N,3] the sample positions actually evaluated (rays entry points only) */
} snerf_field_out;

int snerf_field_forward_points(const snerf_model* m, int variant, int64_t n_points, const float* d_points,
                               int64_t group_size, const float* d_sun, const float* d_classes,
                               const snerf_field_out* out, void* stream);

/* ---- the same on rays: fuses misc.sample_pt_coarse (misc.py:234-247) into the kernel prologue.
 * Rays r = 0..R-1, samples s = 0..S-1, point (r,s) = top[r]*(1-t[s]) + bot[r]*t[s]; d_tvals [S] is the sample
 * parameter vector (linspace + optional shared jitter, built by the caller exactly as the reference does).
 * Ray r uses sun/classes row r / rays_per_group: 1 = per-ray sun and time (training batches), n_rays = one
 * (sun, time) for the whole image (novel-view renders). */
int snerf_field_forward_rays(const snerf_model* m, int variant, int64_t n_rays, int n_samples,
                             const float* d_top, const float* d_bot, const float* d_tvals,
                             int64_t rays_per_group, const float* d_sun, const float* d_classes,
                             const snerf_field_out* out, void* stream);

/* ---- exact solar visibility of secondary rays: All_in_One_Eval._get_exact_solar (Eval_Tools_2.py:255-271) and the
 * `include_exact_solar` block of _internal_render (T_NeRF_Eval_Utils/mg_Img_Eval.py:57-70) as ONE kernel: the density-only
 * network (forward_Classic_Sigma_Only, G_NeRF.py:74-77) over the S samples of every ray with the optical depth kept in
 * registers - no rho [R,S] round trip, no compositing launch:
 *     vis[r] = exp(-sum_{j < S-1} rho(top[r] (1 - t_j) + bot[r] t_j) * ||top[r] - bot[r]|| / S)
 * = PV_Exact[:, -1] of eval_Rho_Only / PV_solar_exact of _internal_render.  d_tvals [S] as for snerf_field_forward_rays
 * (the callers use the end-point-inclusive vector, misc.py:236-239).  flags bit1: a sample outside [-1,1]^3 contributes
 * nothing (mg_Img_Eval.py:65-66; path A leaves it unset).  The model's resolved precision applies (bf16x3 / int8 digits);
 * SNERF_E_INVALID for the bf16 fast mode.  R * S^2 evaluations of the primary image: the default of both renderers
 * (Quick_Run.py:62 use_full_solar=True, mg_Img_Eval.py:96 include_exact_solar=True). */
int snerf_field_ray_visibility(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot,
                               const float* d_tvals, int flags, float* d_vis, void* stream);

/* ---- compositing: Eval_Tools_2.get_PV (:13-16) + PE/PS + albedo / solar shading (:187-215) + depth
 * (mg_run_NeRF.py:188-189).  One wavefront per ray, exclusive prefix by wave shuffles.
 * flags: bit0 = classic solar (Solar_Type_2), bit1 = zero delta for samples outside [-1,1]^3 (mg_Img_Eval.py:42).
 * d_rho_prior (optional [R*S]) with trust in [0,1]: composites rho*trust + rho_prior*(1-trust) (:243), while the
 * solar term keeps using the un-merged PS as the reference does (:229,247). */
typedef struct snerf_composite_out {
    float* d_rgb;        /* [R,3] Rendered_Col */
    float* d_albedo;     /* [R,3] Albedo_Color */
    float* d_pv;         /* [R*S] */
    float* d_pe;         /* [R*S] */
    float* d_ps;         /* [R*S] */
    float* d_delta;      /* [R*S] */
    float* d_shadow;     /* [R] sum_s PS*Solar_Vis */
    float* d_acc;        /* [R] sum_s PS */
    float* d_surf_loc;   /* [R,3] sum PS*pts/(sum PS + 1e-8) */
    float* d_surf_dist;  /* [R] sum cumsum(delta)*PS / sum PS, delta the ray's own segment length (flags bit1 does not shorten the distance) */
} snerf_composite_out;

int snerf_composite_rays(int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                         const float* d_rho, const float* d_col, const float* d_solar_vis, const float* d_sky,
                         int flags, const float* d_rho_prior, float trust,
                         const snerf_composite_out* out, void* stream);
/* The same with the trust factor in DEVICE memory (one float, read when the kernel runs): a training step captured into a hipGraph
 * replays with a trust that changes every step (trust = current_step / n_steps, Eval_Tools_2.py:243) without re-capturing. */
int snerf_composite_rays_dt(int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                            const float* d_rho, const float* d_col, const float* d_solar_vis, const float* d_sky,
                            int flags, const float* d_rho_prior, const float* d_trust,
                            const snerf_composite_out* out, void* stream);

/* ---- one-call render: All_in_One_Eval.eval (Eval_Tools_2.py:165-252, no prior) = group network + field network +
 * compositing.  d_time is [R,4], d_sun [R,3].  d_workspace must hold snerf_render_workspace_bytes(R,S,C) bytes.
 * field/composite outputs are optional extras (NULL structs allowed). */
size_t snerf_render_workspace_bytes(int64_t n_rays, int n_samples, int n_classes);
int snerf_render_rays(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot,
                      const float* d_tvals, const float* d_sun, const float* d_time, int flags,
                      float* d_rgb, const snerf_field_out* field_out, const snerf_composite_out* comp_out,
                      void* d_workspace, size_t workspace_bytes, void* stream);

/* ---- seasonal sweep: mg_Img_Eval.get_imgs_from_Img_Dict (:123-190) and get_imgs_from_Img_Dict_t_step (:192-228).
 * The MLP is NOT re-run: from the per-sample tensors of one render (forward_seperate outputs) produce, for every class
 * vector t of d_class_vecs [T,C]:  season[t,r] = sum_s PS*sigmoid(col_raw + class_t @ adjust)  and
 * shaded[t,r] = season[t,r] * (shadow + (1-shadow)*sky), shadow = sigmoid(30*(sum_s PS*solar_vis - 0.2)).
 * d_sky is ONE vector [3] (the reference uses Sky_Col[0,0]); d_solar_vis may be the estimated or the exact visibility.
 * flags bit1 = zero delta outside the cube.  Also: base [R,3] = sum PS*sigmoid(col_raw), shadow_adjust [R,3],
 * raw_shadow [R].  All outputs optional. */
typedef struct snerf_sweep_out {
    float* d_season;         /* [T,R,3] */
    float* d_shaded;         /* [T,R,3] */
    float* d_base;           /* [R,3] */
    float* d_shadow_adjust;  /* [R,3] */
    float* d_raw_shadow;     /* [R] */
    float* d_classic;        /* [T,R,3] sum_s PS*sigmoid(col_raw + class_t@Adjust)*(SV + (1-SV)*sky): the per-sample shading of
                              * get_imgs_from_Img_Dict(use_classic_shadows=True), mg_Img_Eval.py:165-170 */
} snerf_sweep_out;

/* d_deltas (optional, [R,S]): explicit segment lengths, e.g. the `Deltas` array of a host-side image dict; when given,
 * d_top / d_bot / d_tvals are not read (may be NULL) and flags bit1 is ignored. */
int snerf_composite_sweep(int64_t n_rays, int n_samples, int n_classes, int n_times, const float* d_top,
                          const float* d_bot, const float* d_tvals, const float* d_deltas, const float* d_rho, const float* d_col_raw,
                          const float* d_adjust, const float* d_solar_vis, const float* d_sky, const float* d_class_vecs,
                          int flags, const snerf_sweep_out* out, void* stream);

/* ---- sun walk: many sun directions (and, with the grid compositing below, many seasons) of one view from ONE field pass.
 * The reference renders its season and shadow studies as a grid over view, sun direction and time and calls component_render_by_dir once
 * per (view, sun, time) triple (T_NeRF_Eval_Utils/mg_Season_Eval.py:74-98, Full_Eval_Seasons).  Of the field network only fc_solar_1..4
 * depend on the sun (G_NeRF.py:100-108): the walk runs the trunk, the density / colour head and the colour-adjust branch once per sample and
 * the solar branch once per sun direction.  Exact solar visibility is not part of the walk (every sun direction needs its own secondary
 * rays: snerf_field_ray_visibility), and the int8-digit and one-term bf16 kernel families do not have it.
 *
 * The walk stream of n_suns directions, on the host (no GPU): the field program's stream (program 0 of snerf_model_pack_host; program 3,
 * the K-split order, at width 512) rearranged by whole 16 KiB chunks into [fc1 .. head] [fc_solar_1..4] x n_suns [adjust branch] - the
 * order the walk kernels' weight ring consumes.  stream_out may be NULL to query the size.  SNERF_E_INVALID unless 1 <= n_suns <= 32. */
int snerf_model_pack_sun_walk_host(snerf_model* m, int n_suns, uint8_t* stream_out, size_t* stream_bytes);
/* The walk on rays (the device side of `_internal_render`, mg_Img_Eval.py:17-56, for n_suns sun directions of one view): points as in
 * snerf_field_forward_rays, ONE class vector d_classes [C] (may be NULL) for the whole launch, d_suns [n_suns,3].  Outputs as
 * snerf_field_out (all optional), stored once per point - except out->d_solar_vis, which is [n_suns, R*S]: row j is what
 * snerf_field_forward_rays gives for sun j, bit for bit.  SNERF_E_INVALID unless the model's resolved precision is SNERF_PREC_BF16X3
 * (width 64, 256 or 512) and 1 <= n_suns <= 32.  The device copy of the walk stream is built at the first call per n_suns and kept
 * (the most recent one) until the model is destroyed. */
int snerf_field_sun_walk_rays(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot,
                              const float* d_tvals, int n_suns, const float* d_suns, const float* d_classes,
                              const snerf_field_out* out, void* stream);
/* Grid compositing of a walk: `Season_Adj_Img * Shadow_Adjust` of Full_Eval_Seasons (mg_Season_Eval.py:74-98; mg_Img_Eval.py:192-228 per
 * (sun, time)) for M sun directions x T class vectors from the per-sample tensors of one walk.  As snerf_composite_sweep (same PS, same
 * flags, top / bot / tvals or explicit d_deltas), with d_solar_vis [M,R,S] and d_sky [M,3]:
 *   season[k,r] = sum_s PS sigmoid(col_raw + class_k @ adjust),  raw_shadow[j,r] = sum_s PS solar_vis[j,r,s],
 *   shadow_adjust[j,r] = m + (1 - m) sky_j with m = sigmoid(30 (raw_shadow[j,r] - 0.2)),  shaded[j,k,r] = season[k,r] * shadow_adjust[j,r].
 * All outputs optional.  SNERF_E_INVALID when a ray's PS and shadow factors (4 (S + 3 M) floats per workgroup) exceed 64 KiB of LDS. */
typedef struct snerf_sun_walk_out {
    float* d_shaded;         /* [M,T,R,3] */
    float* d_season;         /* [T,R,3] */
    float* d_base;           /* [R,3] sum_s PS sigmoid(col_raw) */
    float* d_raw_shadow;     /* [M,R] */
    float* d_shadow_adjust;  /* [M,R,3] */
} snerf_sun_walk_out;
int snerf_composite_sun_walk(int64_t n_rays, int n_samples, int n_classes, int n_times, int n_suns, const float* d_top,
                             const float* d_bot, const float* d_tvals, const float* d_deltas, const float* d_rho, const float* d_col_raw,
                             const float* d_adjust, const float* d_solar_vis, const float* d_sky, const float* d_class_vecs,
                             int flags, const snerf_sun_walk_out* out, void* stream);

/* ---- ray surface: height maps from a density-only ray pass with the compositing inside the field kernel.
 * The reference forms its height maps from the density along a ray alone: Quick_Run_Net.get_DSM (Quick_Run.py:207-226, :37-40),
 * Eval_funcs.eval_HM / gen_results (T_NeRF_Eval_Utils/Eval_funcs.py:268-319) and the surface location / distance of Net_tool.eval_img
 * (mg_run_NeRF.py:188-189).  One launch walks the S samples of every ray from t = 0 (d_top) to d_bot, 32 per pass, through the density-only
 * network and the transmittance scan of snerf_composite_rays, and stores four numbers per ray, d_out [n_rays,4] (16-byte aligned):
 *   [0] acc   = sum_s PS_s                       the opacity; Est_HM's denominator (Eval_funcs.py:319), the quotients of mg_run_NeRF.py:188-189
 *   [1] mt    = sum_s PS_s t_s                   surface location = (top (acc - mt) + bot mt) / (acc + 1e-8)        (mg_run_NeRF.py:188)
 *   [2] mi    = sum_s PS_s s                     height = acc - 2 mi / (S - 1) = sum_s PS_s linspace(1, -1, S)[s]   (Quick_Run.py:39, Eval_funcs.py:319);
 *                                                surface distance = delta (mi + acc) / acc                          (mg_run_NeRF.py:189)
 *   [3] carry = sum of rho_s delta_s walked      transmittance behind the walked samples = exp(-carry)
 * with PS_s = exp(-sum_{j<s} rho_j delta_j) (1 - exp(-rho_s delta_s)), delta = ||top - bot|| / S, all S samples counting.
 * flags bit1 = a sample outside [-1,1]^3 gets delta 0; bit2 = no early-out.  Early-out: once every ray of a workgroup has walked past
 * optical depth 18 its remaining passes are skipped (every PS left is below exp(-18) = 1.5e-8); carry then holds the depth walked.
 * SNERF_E_INVALID for bad arguments and unless the model's resolved precision is SNERF_PREC_BF16X3 (width 64, 256 or 512). */
int snerf_field_ray_surface(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot,
                            const float* d_tvals, int flags, float* d_out, void* stream);

/* ---- shadow walk: the reference's shadow test with the sun-ray walk scored inside the field kernel.
 * The reference ends an evaluation by comparing, sample by sample along rays laid through ground points towards the sun, the solar visibility the network
 * has learned with the one its own density implies: eval_shadow_data and shadow_anaylysis (T_NeRF_Eval_Utils/mg_Shadow_Eval.py:72-104,134-163).  One launch
 * walks the S samples of every ray from t = 0 (d_top) to d_bot, 32 per pass, through the trunk, the density head and fc_solar_1..4 with the ray's own sun
 * direction d_sun [n_rays,3] (not normalised here: the vector goes into the encoding as the caller gives it), forms
 *   PV_s  = exp(-sum_{j<s} rho_j delta_j)        the exact visibility, get_PV's exclusive prefix (delta = ||top - bot|| / S, all S samples counting)
 *   vis_s = sigmoid(fc_solar_4)                  the learned one
 *   PS_s  = PV_s (1 - exp(-rho_s delta_s))
 * and stores eight numbers per ray, d_out [n_rays,8] (32-byte aligned):
 *   [0] number of samples with PV > .5 and vis > .5      [1] with PV > .5      [2] with vis > .5          (floats holding integers)
 *   [3] sum_s (PV_s - vis_s)^2       [4] sum_s |PV_s - vis_s|       [5] sum_s PS_s vis_s       [6] sum_s PS_s       [7] sum_s rho_s delta_s
 * The sums over rays, and the scores formed from them, are the caller's.  flags bit1 = a sample outside [-1,1]^3 gets delta 0
 * (deltas[Zero_Tool(Xs)] = 0); no other bit is read, and there is no early-out: the learned visibility behind a surface is scored like any other.
 * SNERF_E_INVALID for bad arguments and unless the model's resolved precision is SNERF_PREC_BF16X3 (width 64, 256 or 512). */
int snerf_field_shadow_walk(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_sun,
                            const float* d_tvals, int flags, float* d_out, void* stream);

/* ---- solar audit: the learned sun visibility against the one the density implies, scored inside the field kernel.
 * The reference ends a study of a trained scene by rendering each (view, sun) pair with component_render_by_dir(include_exact_solar=True) and comparing, sample
 * by sample, Est_Solar_Vis with Exact_Solar (T_NeRF_Eval_Utils/mg_Advanced_Solar.py eval_solar_data; the exact block is mg_Img_Eval.py:57-70).  One launch takes
 * the primary rays of a view (d_top, d_bot [n_rays,3], d_tvals [S]) and ONE sun direction sun3 (three doubles in HOST memory, read before the launch), forms for
 * every sample s of every ray the secondary ray towards the sun
 *   p = top (1 - t_s) + bot t_s,   K = (1 - p_z) / (float)sun_z (fp32),   top2 = (float)((double)p + (double)K sun3),   bot2 = p,
 * walks its S samples from the point outwards, 32 per pass, through the density-only network and scores
 *   E_s = exp(-sum_{j<S-1} rho_j delta2)         the exact visibility (delta2 = ||top2 - bot2|| / S; the last sample never counts)
 * against the caller's V = d_est_vis [n_rays,S] (the learned visibility, e.g. of the sun walk) and PS = d_ps [n_rays,S] (snerf_composite_rays).  Per primary
 * ray d_out [n_rays,8] (32-byte aligned):
 *   [0] number of samples with E > .5 and V > .5      [1] with E > .5      [2] with V > .5          (floats holding integers)
 *   [3] sum_s E_s PS_s       [4] sum_s V_s PS_s       [5] sum_s PS_s       [6] sum_s (E_s - V_s)^2       [7] sum_s |E_s - V_s|
 * From [0..2] and S follow TP / FP / FN / TN of All_Solar_Vis, from [3] and [4] against .3 those of Surface_Solar_Vis.  d_exact [n_rays,S] (may be NULL)
 * receives E per sample, the reference's Exact_Solar; it equals snerf_field_ray_visibility on the same secondary rays.  The sums are added in a fixed order:
 * two launches give the same bits.  flags bit1 = a sample of a secondary ray outside [-1,1]^3 gets delta 0; bit2 = no early-out; any other bit is refused.
 * Early-out: once every secondary ray of a workgroup's group of samples has passed optical depth 18 the group's remaining passes are skipped (E < exp(-18)).
 * SNERF_E_INVALID, before anything is launched, for a NULL required pointer, n_rays < 0, n_samples < 1, a sun that is not finite or has sun_z <= 0, d_out
 * off 32 bytes, and unless the model's resolved precision is SNERF_PREC_BF16X3 (width 64, 256 or 512).  n_rays == 0 succeeds and launches nothing. */
int snerf_field_solar_audit(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                            const double* sun3 /* host */, const float* d_est_vis, const float* d_ps, int flags, float* d_out, float* d_exact,
                            void* stream);

/* ---- frame walk: the frames of the reference's fly-through films with the shading and compositing inside the field kernel.
 * The reference renders a film frame from a slab of parallel rays (sample_rays_projective, T_NeRF_Eval_Utils/mg_movie_maker.py:52-70): T_NeRF.forward on
 * every sample, the density zeroed outside the cube, and a compositing of its own with the learned visibility applied per sample (get_Img.eval_rays,
 * :108-177; eval_rays_advanced re-runs the network once per season shown, :179-187).  One launch walks the S >= 2 samples of every ray from d_top (t = 0) to
 * d_bot, 32 per pass, through the whole field network - trunk, head, fc_solar_1..4, the colour-adjust branch - and forms, with the frame's one `delta`
 * (||top - bot|| / (S - 1), the spacing of end-point-inclusive samples; d_tvals holds t_s = s / (S - 1)),
 *   PS_s    = exp(-sum_{j<s} rho_j delta) (1 - exp(-rho_s delta))
 *   vis_s   = sigmoid(fc_solar_4),   shade_s = vis_s + (1 - vis_s) sky
 *   col_k,s = sigmoid(col_raw_s + class_vecs[k] @ adjust_s)            for the n_times seasons, 1 <= n_times <= 4: only the class vector depends on the time
 * and stores sixteen numbers per ray, d_out [n_rays,16] (64-byte aligned):
 *   [3k .. 3k+2] sum_s PS_s shade_s col_k,s   (Out_Img of season k, :153-161; 0 for k >= n_times)
 *   [12] sum_s PS_s        [13] sum_s PS_s s   (HM = 2 [13] / (S - 1), :185-186)        [14] optical depth walked        [15] sum_s PS_s vis_s
 * The same for every ray of the launch, all in device memory: d_sun [3] (into the encoding as given), d_sky [3] (sigmoided: it depends on the sun only),
 * d_class_vecs [n_times, C].  flags bit1 = a sample outside [-1,1]^3 gets delta 0 (Rho[Zero_Tool(Xs)] = 0, :141); bit2 = no early-out: otherwise a
 * workgroup whose rays have all passed optical depth 18 skips their remaining passes (every further PS < exp(-18)).
 * SNERF_E_INVALID for a NULL input, n_rays < 0, n_samples < 2, n_times outside 1..4, a delta that is not finite and positive, a d_out off 64 bytes, and
 * unless the model's resolved precision is SNERF_PREC_BF16X3 (width 64, 256 or 512). */
int snerf_field_frame_walk(const snerf_model* m, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals, float delta,
                           const float* d_sun, const float* d_sky, int n_times, const float* d_class_vecs, int flags, float* d_out, void* stream);
#define SNERF_MAX_FRAME_TIMES 4

/* ---- training engine: the device side of Net_tool.train_step (mg_run_NeRF.py:288-326) = All_in_One_Eval.get_loss
 * (Eval_Tools_2.py:340-459) forward passes in .train() mode, backward, Adam.  Layer-wise, fp32 storage, 3-term split bf16 MFMA
 * GEMMs (exact-fp32 MFMA under SNERF_TRAIN_GEMM=fp32), batch-statistics BatchNorm1d (momentum 0.01, misc.py:170) with running-stat EMA, activations stashed in HBM.
 * Two passes per step, as the reference: image rays (everything gets a gradient except the solar branch, whose output
 * is detached, Eval_Tools_2.py:214) and random sun rays (forward_Solar: trunk without gradient, :297-337).
 * The caller owns all memory: a flat parameter arena and same-sized gradient / Adam arenas (layout from
 * snerf_trainer_tensor_info: state_dict keys -> offset), the BatchNorm running-stat arena, and the workspace.
 * The scalar loss terms stay with the caller: forward returns Rendered_Col / Albedo / Sky_Col / Solar_Vis ..., backward
 * takes dL/d(those). */
typedef struct snerf_trainer snerf_trainer;
snerf_trainer* snerf_trainer_create(int layer_width, int n_classes);
void snerf_trainer_destroy(snerf_trainer* t);
/* class count of a live trainer; -1 if `t` is not one (never created by this library, or already destroyed): handle validation for
 * callers that carry the pointer as an integer (torch.ops.season_nerf.train_*; no reference counterpart - the reference's trainer is
 * a Python object, Net_Tool_2.py:11-61). */
int snerf_trainer_classes(const snerf_trainer* t);
int64_t snerf_trainer_param_floats(const snerf_trainer* t);
int64_t snerf_trainer_buffer_floats(const snerf_trainer* t);
int snerf_trainer_tensor_count(const snerf_trainer* t);
int snerf_trainer_tensor_info(const snerf_trainer* t, int index, char* key, int key_cap, int* is_buffer, int64_t* offset,
                              int64_t* numel, int* rows, int* cols);
size_t snerf_trainer_workspace_bytes(snerf_trainer* t, int64_t n_rays, int64_t n_solar_rays, int n_samples);
int snerf_trainer_bind(snerf_trainer* t, float* d_params, float* d_grads, float* d_adam_m, float* d_adam_v, float* d_buffers,
                       void* d_workspace, size_t workspace_bytes, int64_t n_rays, int64_t n_solar_rays, int n_samples);
/* the sizes the trainer is bound to (any pointer may be NULL); SNERF_E_STATE before snerf_trainer_bind */
int snerf_trainer_bound_sizes(const snerf_trainer* t, int64_t* n_rays, int64_t* n_solar_rays, int* n_samples);
/* image-ray pass: T_NeRF.forward + compositing.  train_bn: 1 = batch statistics + EMA update, 0 = running statistics.
 * The pass remembers which it was, and its backward (snerf_trainer_backward_image / _dt / _points) differentiates the function that ran:
 * after train_bn = 1 the BatchNorm layers give dz = gamma istd (dy - mean(dy) - xhat mean(dy xhat)), after train_bn = 0 (frozen BatchNorm:
 * mean and istd are constants) dz = gamma istd dy, and the biases in front of BatchNorm get a gradient.  d gamma = sum dy xhat and
 * d beta = sum dy in both, xhat from the statistics of the forward.  A train_bn = 0 pass and its backward leave the running statistics alone
 * and need no collective (snerf_trainer_set_allreduce: none is issued).
 * flags: bit0 = classic solar as in snerf_composite_rays.  bit1 (zero segment length outside the cube) is refused with SNERF_E_INVALID:
 * the compositing backward differentiates the plain segment length, so a forward with bit1 would get the gradients of another function. */
int snerf_trainer_forward_image(snerf_trainer* t, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot,
                                const float* d_tvals, const float* d_sun, const float* d_time, int train_bn, int flags,
                                const snerf_composite_out* out, float* d_sky, float* d_classes,
                                const snerf_field_out* per_sample, void* stream);
/* gradients of the image pass: dL/dRendered_Col [R,3] (opt), dL/dAlbedo_Color [R,3] (opt), dL/dSky_Col per ray [R,3] (opt),
 * dL/dPE [R*S] (opt); DSM-prior phase (Eval_Tools_2.py:218-248): d_rho_prior [R*S] + trust and the gradients of
 * Rendered_Col_Merged / the merged Albedo_Color (opt).  ACCUMULATES into the gradient arena. */
int snerf_trainer_backward_image(snerf_trainer* t, const float* d_g_rgb, const float* d_g_albedo, const float* d_g_sky,
                                 const float* d_g_pe, const float* d_rho_prior, float trust, const float* d_g_rgb_merged,
                                 const float* d_g_albedo_merged, void* stream);
/* The same with the trust factor in device memory (see snerf_composite_rays_dt). */
int snerf_trainer_backward_image_dt(snerf_trainer* t, const float* d_g_rgb, const float* d_g_albedo, const float* d_g_sky,
                                    const float* d_g_pe, const float* d_rho_prior, const float* d_trust, const float* d_g_rgb_merged,
                                    const float* d_g_albedo_merged, void* stream);
/* Seam B1 in train mode - `T_NeRF.forward(X, Solar_Angle, Time)` called on points with an autograd graph attached
 * (T_NeRF_net_v2.py:75-105, called so by the reference's evaluator at Eval_Tools_2.py:174-176): backward of the last
 * snerf_trainer_forward_image from gradients with respect to the PER-SAMPLE network outputs - dL/dRho [N], dL/dCol [N,3],
 * dL/dSolar_Vis [N], dL/dSky_Col per ray [R,3], dL/dclasses per ray [R,C]; each optional (NULL = zero).  ACCUMULATES into the
 * gradient arena like snerf_trainer_backward_image. */
int snerf_trainer_backward_points(snerf_trainer* t, const float* d_g_rho, const float* d_g_col, const float* d_g_solar_vis,
                                  const float* d_g_sky, const float* d_g_classes, void* stream);
/* sun-ray pass: T_NeRF.forward_Solar + PV_Exact / PE (end-point sampling is the caller's d_tvals). */
int snerf_trainer_forward_solar(snerf_trainer* t, int64_t n_rays, int n_samples, const float* d_top, const float* d_bot,
                                const float* d_tvals, const float* d_sun, int train_bn, float* d_solar_vis, float* d_pv,
                                float* d_pe, float* d_sky_raw, float* d_rho, float* d_points, float* d_delta, void* stream);
int snerf_trainer_backward_solar(snerf_trainer* t, const float* d_g_solar_vis, void* stream);
int snerf_trainer_zero_grad(snerf_trainer* t, void* stream);
/* Data-parallel training with BatchNorm statistics over the GLOBAL batch (what the single-process reference computes on the
 * concatenated rays; `nn.BatchNorm1d` in misc.SineLayer, misc.py:169-170).  `fn` must sum `count` elements of the device
 * buffer `d_buf` (float when is_double == 0, double otherwise) over all ranks, in stream order on `stream`, and return 0.
 * The engine calls it for the per-layer statistics in forward (2 x n_out doubles) and the two BatchNorm backward sums
 * (2 x W floats); every rank must run the same shapes (equal ray shards).  fn == NULL restores per-rank statistics. */
typedef int (*snerf_allreduce_fn)(void* user, void* d_buf, int64_t count, int is_double, void* stream);
int snerf_trainer_set_allreduce(snerf_trainer* t, snerf_allreduce_fn fn, void* user, int world_size);
/* ---- the three products of a Linear / SineLayer (`misc.SineLayer.forward`, misc.py:188-194, and its autograd backward) as
 * stand-alone calls - the building blocks of the training engine, exposed for tests and for callers that schedule layers
 * themselves.  Row-major fp32, leading dimensions in floats; weight is the [n_out, n_in] nn.Linear matrix.
 * precision: 1 = error-compensated bf16x3 MFMA (~1e-5 relative, needs d_scratch of snerf_linear_scratch_bytes), 0 = exact
 * fp32 MFMA.  Thin heads: with precision == 1, n_out <= 4 and n_points >= 1024, forward and wgrad do not use the MFMA kernels but
 * stream over `in` in EXACT fp32, as the training engine does for its colour / density / visibility heads.  The forward does
 * so only when a bias is given and d_stats is NULL (the stream always adds the bias and has no statistics epilogue).  Both do
 * so only where the stream takes the layout (n_in a multiple of 4, at most 256 for the forward and 1024 for wgrad; `in` 16-byte
 * aligned; ld_in a multiple of 4) and while SNERF_FUSED_HEADS (forward) / SNERF_THIN_WGRAD (wgrad) is not 0; otherwise bf16x3 as
 * above.  dgrad never streams.  Arguments are checked the same way on every route, before one is chosen.
 *   forward: out[m, o] = alpha * (sum_i in[m, i] * weight[o, i] + bias[o]);  d_stats (optional, bf16x3 only, caller-zeroed
 *            double[2][n_out]) += sum_m (out - alpha*bias), sum_m (out - alpha*bias)^2   (train-mode BatchNorm statistics)
 *   dgrad:   grad_in[m, i] (+)= alpha * sum_o grad_out[m, o] * weight[o, i]   for i < n_cols
 *   wgrad:   grad_weight[o, i] += alpha * sum_m grad_out[m, o] * in[m, i]     (always accumulates)
 * Activation on load (bf16x3 only; forward and wgrad): with d_act_tab != NULL the first act_cols columns of `in` are taken as the
 * stored PRE-activation z of the SineLayer below and become sin(2 pi (a z + b)) in registers (one fma + one v_sin_f32);
 * d_act_tab holds [a | b], each act_cols floats, with BatchNorm and the 1/(2 pi) folded in: a = gamma*istd/(2 pi),
 * b = (beta - gamma*mu*istd)/(2 pi)  (a = 1/(2 pi), b = 0 without BatchNorm); forward needs act_cols % 8 == 0.
 * The training engine uses this so that post-activations are never written to HBM.
 * Activation backward in the dgrad epilogue (bf16x3; with `accumulate` this call must be the last producer): with d_below_z != NULL, grad_in is dL/dH of the SineLayer
 * below, whose pre-activation is d_below_z [n_points, ld_below_z] and table d_below_tab ([a | b], n_cols each); what is written
 * is dL/dH * cos(2 pi (a z + b)), and d_sums (caller-zeroed double[2][n_cols]) += sum_m of it and of it times
 * xhat = (z - mu)*istd (d_below_mu / d_below_istd, NULL for a layer without BatchNorm: second sum 0). */
size_t snerf_linear_scratch_bytes(int n_out, int n_in);
int snerf_linear_forward(int64_t n_points, int n_in, int n_out, const float* d_in, int64_t ld_in, const float* d_weight,
                         const float* d_bias, float alpha, float* d_out, int64_t ld_out, double* d_stats, int precision,
                         void* d_scratch, size_t scratch_bytes, const float* d_act_tab, int act_cols, void* stream);
int snerf_linear_dgrad(int64_t n_points, int n_in, int n_out, const float* d_grad_out, int64_t ld_go, const float* d_weight,
                       int n_cols, float alpha, int accumulate, float* d_grad_in, int64_t ld_gi, int precision,
                       void* d_scratch, size_t scratch_bytes, const float* d_below_z, int64_t ld_below_z,
                       const float* d_below_tab, const float* d_below_mu, const float* d_below_istd, double* d_sums,
                       void* stream);
int snerf_linear_wgrad(int64_t n_points, int n_in, int n_out, const float* d_grad_out, int64_t ld_go, const float* d_in,
                       int64_t ld_in, float alpha, float* d_grad_weight, int precision, const float* d_act_tab, int act_cols,
                       void* stream);
/* test introspection: synchronous copy of an internal buffer ("d_rho", "d_col", "d_head", "d_sky", "d_sv_raw", "rho", "col", "sv", "sky", ...)
 * to the host.  "d_sv_raw": dL/dSolar_Vis of the classic solar model, as the pre-sigmoid gradient the network backward consumed. */
int snerf_trainer_debug_read(snerf_trainer* t, const char* name, float* host_out, int64_t n_floats);
/* test introspection: ONE launcher of the training engine's element kernels (csrc/train.h, csrc/train_kernels.hip) on the caller's device buffers, without
 * a trainer.  op names the launcher; sizes (counts, leading dimensions and flags), scalars and device pointers come in the order given below and in
 * exactly these numbers.  Everything the launcher takes on trust is checked BEFORE any HIP call - required pointers non-null (and 4-byte aligned, the
 * double sums 8-byte), counts non-negative, leading dimensions >= column counts, 1 <= n_classes <= 8 for the point outputs, K <= 4 and thin_dgrad_ok for
 * the thin input gradient - otherwise SNERF_E_INVALID with a message and nothing is launched (no GPU is needed to be refused).  Asynchronous on `stream`.
 * Returns a negative SNERF_E_* code or the kernel the launcher chose (its own decision, not a restatement of it):
 *    0 pe_points_kernel          1 pe_small_kernel            2 colreduce_kernel           3..6 colpass_vec_kernel<1..4>
 *    7 bn_bwd2_kernel            8 bn_finalize_kernel         9 bn_finalize_shifted_kernel 10 act_sums_finalize_kernel
 *   11 act_table_kernel         12 sin_fwd_kernel            13 sin_fwd_vec_kernel         14 thin_dgrad_kernel<false>
 *   15 thin_dgrad_kernel<true>  16 point_out_fwd_kernel      17 point_out_bwd_kernel       18 softmax_kernel
 *   19 softmax_bwd_kernel       20 sigmoid_kernel            21 sigmoid_bwd_kernel         22 colsum_kernel
 *   23 copy_cols_kernel         24 bcast_rows_kernel         25 reduce_rows_kernel         26 fill_zero_kernel
 *   27 copy_f32_kernel          28 fill_zero_bytes_kernel    29 copy_bytes_kernel
 *   30..39 wgrad_bf16x3_kernel<FULL, BNZ, TA, TB> (csrc/gemm.hip): 30 <F,F,1,2>  32 <F,F,2,2>  34 <F,F,1,4>  36 <F,F,2,4>  38 <T,F,2,4>, the odd number
 *         after each the same block shape with BNZ (the BatchNorm ride)
 *   40 thin_wgrad_kernel<false> 41 thin_wgrad_kernel<true>   42 thin_fwd_kernel<false>     43 thin_fwd_kernel<true>    (<true>: activation on load)
 * "wgrad" returns more than a kernel number - one byte per launch, the first launch in the low byte, the second byte 0 when there was one launch:
 *         kernel (30..39) | partial << 6 | reverse << 7;  partial: two-stage reduction through the partial-sum scratch (else fp32 atomics), reverse: the
 *         stages ran from the last to the first (the direction's turn, taken from 32768 rows on).  Two launches: a BatchNorm layer with n_in > 256.
 * Operations - sizes | scalars | pointers ("?" = may be NULL):
 *   pe_points            n, n_samples, ld2 | - | points?, top?, bot?, tvals?, pe, pts?, pe2?     (points, or top + bot + tvals with n_samples | n)
 *   pe_small             rows, in_stride, n_dims, n_freq, out_stride | - | in, out
 *   colreduce            mode (0..2), M, C, ld, ldd (0 = ld) | alpha0 | Z, D?, mu?, istd?, gamma?, beta?, out0, out1?   (mode 1 needs all, mode 2 needs D)
 *   bn_bwd2              M, C, ld, ldd, M_global (>= M), d_is_dy | alpha | Z, D, mu, istd, gamma, beta, sdy, sdyx, dbias?
 *   bn_finalize          M, C, stage (0..2) | - | colsum?, m2?, mean?, istd?, running_mean?, running_var?   (what the stage reads and writes)
 *   bn_finalize_shifted  M, C | alpha | stats, bias, mean, istd, running_mean, running_var, gamma?, beta?, tab?
 *   act_sums_finalize    C | scale0 | stats, out0?, out1?, acc0?, acc1?
 *   act_table            n | - | mu?, istd?, gamma?, beta? (all or none), dst
 *   sin_fwd              M, C, ldz, ldh | - | Z, H, mu?, istd?, gamma?, beta? (all or none)
 *   thin_dgrad           M, N, K, ldd, ldw, ldc, accumulate, eld | alpha | D, W, W3?, C, ez?, etab?, emu?, eistd?, stats?
 *   wgrad                M, n_out, n_in, ldz, ldi, ldw, tab_cols, ldzz, M_global, route (1) | alpha, bias_alpha | dZ, In, dW, tab?, z?, gamma?, mu?, istd?, sdy?,
 *                        sdyx?, dbias?   - the weight gradient as the engine issues it: a Product through run_wgrad on the Rows route (csrc/linear_product.h),
 *                        dW [n_out, ldw] += alpha dZ^T H, H = In with sin(2 pi (a In + b)) over its first tab_cols columns (tab = [a | b], tab_cols each;
 *                        tab and tab_cols go together).  z .. sdyx (all or none) are the BatchNorm block: dZ [M, ldz] holds dL/dY on entry and
 *                        dL/dZ = gamma istd (dY - sdy / M_global - xhat sdyx / M_global) on exit, z [M, ldzz] is the pre-activation, dbias (optional) +=
 *                        bias_alpha sum_m dZ; with n_in > 256 the layer goes as two launches (256 columns with the block, the rest on the finished dZ).
 *                        Refused: leading dimensions below their column counts or (ldz, ldi, ldzz) from 2^24 on, a partial BatchNorm block, M_global < M,
 *                        a ride that would not get one block over the inputs, route 0 (the exact fp32 GEMM: it takes neither a table nor the block, and has
 *                        no kernel number - snerf_linear_wgrad runs it).
 *   thin_wgrad           M, N, K, ldd, ldi, ldw, tab_cols | alpha | D, In, dW, dW3?, tab?      dW [K, ldw] += alpha D[:, :K]^T H; dW3 (K = 4 only): row 3
 *                        of the result is added there instead (two heads as one product).  N a multiple of 4 in 4..1024, ldi a multiple of 4, In on 16 bytes.
 *   thin_fwd             M, N, K, ldi, ldw, ldo, tab_cols | alpha | In, W, W3?, bias, bias3?, Out, tab?   Out [M, ldo][:, :K] = alpha (H W^T + bias); W3 / bias3
 *                        (K = 4 only): row 3 of W / element 3 of bias are read there instead.  N a multiple of 4 in 4..256, ldi a multiple of 4, In on 16 bytes.
 *                        Under a dry run (snerf_rows_debug_set) these three check their arguments, plan and return as always, launch nothing and read no
 *                        pointer; a dry run's plan reports the direction the next launch will get and does not take its turn.
 *   point_out_fwd / point_out_bwd   n, n_samples, n_classes | - | head, adj, sv_raw, cls, rho, col, sv, adjust_col, d_rho, d_col, d_sv, d_head, d_adj, d_cls,
 *                        d_sv_raw   (each optional as the kernels allow)
 *   softmax              rows, C | - | logits, p             softmax_bwd   rows, C | - | p, dp, dlogits
 *   sigmoid              n | - | x, y                        sigmoid_bwd   n | - | y, dy, dx
 *   colsum               M, C, ld | alpha | X, out           copy_cols     M, C, ld_src, ld_dst, accumulate | - | src, dst
 *   bcast_rows           n, n_samples, C, ld_dst, col0 | - | src, dst      reduce_rows   n_groups, n_samples, C, ld_src, col0 | - | src, dst
 *   fill_zero            n | - | p                           copy_f32      n | - | dst, src
 *   fill_zero_bytes      bytes | - | p                       copy_bytes    bytes | - | dst, src
 *   colpass_rows_per_block  M, C | - | -   and   thin_dgrad_rows_per_block  M, N | - | -   launch nothing: they return the rows one block (one chunk)
 *                        of colpass_vec_kernel / thin_dgrad_kernel walks at this shape, as the launcher derives it. */
int snerf_train_kernel_debug(const char* op, const int64_t* sizes, int n_sizes, const float* scalars, int n_scalars, void* const* d_ptrs, int n_ptrs,
                             void* stream);
/* test introspection of the bf16x3 row GEMMs' routing (csrc/gemm.hip plan_gemm_rows: which of the separately compiled kernel instances a product runs on).
 * snerf_rows_debug_set - state of the CALLING THREAD, (NULL, 0, 0) restores the default:
 *   switches8: NULL = the process's own environment switches, else eight ints that replace them for every reader - SNERF_GEMM_AREG, SNERF_GEMM_AREG_ACT,
 *              SNERF_AREG_HV, SNERF_GEMM_FULL, SNERF_GEMM_PF, SNERF_GEMM16, SNERF_GEMM16_K320, SNERF_SNAKE, in this order;
 *   dry_run:   snerf_linear_forward / snerf_linear_dgrad (and the weight-gradient operations of snerf_train_kernel_debug) check their arguments and route as always; the route - and on the row-GEMM route the plan - is
 *              recorded, nothing is launched and no pointer is dereferenced (any aligned non-null addresses will do: no GPU is needed);
 *   x_padded:  the public calls promise that the input's columns n_in .. the next multiple of 16 exist (ld_in covers them) and hold zeros, as the engine
 *              does for its K = 63 / 319 / 575 inputs.
 * snerf_rows_record_reset / _read - one record per PROCESS (the engine's backward may run on another thread): the distinct plans executed or dry-run
 * since the last reset.  reset(on) empties it and switches recording of executed plans on or off (dry runs are always recorded).  read copies at most
 * max_entries entries of 12 ints and returns how many the record holds: route (0 thin-head stream, 1 row GEMM, 2 exact-fp32 GEMM), then for a row GEMM
 * (otherwise kernel = -1, rest 0) kernel (0 gemm_areg_kernel, 1 gemm_rows16_kernel, 2 gemm_rows_full_kernel, 3 gemm_rows_kernel), the template arguments
 * nt, pf, aol, act, hv, then tab_lds, zero_bn, the weights' split layout (0 Tile32, 1 Tile16, 2 KMajor32), grid, dynamic LDS bytes. */
int snerf_rows_debug_set(const int* switches8, int dry_run, int x_padded);
int snerf_rows_record_reset(int on);
int snerf_rows_record_read(int32_t* host_out, int max_entries);
/* torch.optim.Adam semantics (no weight decay) over the whole parameter arena in one launch; step counts from 1. */
int snerf_trainer_adam_step(snerf_trainer* t, float lr, float beta1, float beta2, float eps, int step, void* stream);
/* the same update with its per-step scalars in DEVICE memory: d_hyper6 = [lr, beta1, beta2, eps, 1 - beta1^step, 1 - beta2^step].  For a training
 * step captured in a hipGraph (kernel arguments are frozen at capture): the host rewrites the six floats before every replay (OneCycleLR,
 * Net_Tool_2.py:123-130; Adam's bias corrections). */
int snerf_trainer_adam_step_dev(snerf_trainer* t, const float* d_hyper6, void* stream);
/* ---- the scalar loss terms of a training step: All_in_One_Eval.get_loss, Eval_Tools_2.py:340-450, solar rays on (:350-372), default solar model: the MSE
 * colour loss (:413) or Barron's adaptive colour loss (:421-450), without or with the DSM-prior phase (:243, :391-412).  flags selects the configuration;
 * the value vector follows get_loss's key order:
 *   0                                      (5):  Solar_Correction (:361), Solar_Correction_2 (:366, a value only: detached), Sky_Color_Var (:381-388),
 *                                                Albedo_Color (:374-379), Color (:413)
 *   SNERF_LOSS_ADAPTIVE                    (8):  Solar_Correction, Solar_Correction_2, Sky_Color_Var, Albedo_Color, Color_ada, Color_alpha, Color_width, Color
 *   SNERF_LOSS_ADAPTIVE | SNERF_LOSS_PRIOR (12): Solar_Correction, Solar_Correction_2, Sky_Color_Var, Albedo_Color, Alpha_Adjust_ada, Color_ada, Color_alpha,
 *                                                Color_width, Alpha_Adjust, Alpha_alpha, Alpha_width, Color
 *   SNERF_LOSS_PRIOR                       (6):  Solar_Correction, Solar_Correction_2, Sky_Color_Var, Albedo_Color, Color, Alpha_Adjust
 * SNERF_LOSS_SKY_DETACHED: Sky_Color_Var is a value only (the reference detaches it in the prior phase).  d_sky is the per-ray sky colour [R,3] (the
 * reference's [R,S,3] tensor holds S copies of it).  Color_ada = mean over [R,3] of
 * nll(Rendered_Col - GT) with nll(x) = rho(x, alpha, c) + log c + log Z(alpha) (Barron 2019, as season_nerf_amd/adaptive_loss.py states it; parity with
 * robust_loss_pytorch is NOT pinned); Alpha_Adjust_ada = mean over [R,S] of nll(PE - PE_Supervised) under the second, one-dimensional loss object;
 * Alpha_Adjust = MSE(PE, PE_Supervised); Color = MSE(d_rgb_merged if given, else d_rgb, GT) - a value only beside the adaptive loss.  alpha / scale are
 * the float32 vectors the caller formed ([3] for colour, [1] for alpha); log Z is the cubic Hermite spline on d_logz_value / d_logz_slope: 513 float64 numbers
 * each on the grid alpha_i = 4 i / 512 (float64: rounding the table to float32 alone moves d log Z / d alpha by 1.5e-5).  Pointers a configuration does not use may be NULL.
 * d_albedo_min_global (optional, [3]) + world: data-parallel training - the minimum over the global batch (one MIN all-reduce by the caller), the
 * Albedo_Color value divided by n_rays * world.
 * forward: d_vals and d_weights hold snerf_loss_all_term_count(flags) floats - the weights of sum(value * weight): w_solar / mean(scale colour)^2 for the
 * two Solar_Correction terms beside the adaptive loss (w_solar otherwise), w_solar for Sky_Color_Var and Albedo_Color, w_color for Color_ada / Color,
 * w_alpha for Alpha_Adjust(_ada), 1 for the logged means; d_aux14: 14 floats for the backward - the per-channel albedo minimum the Albedo_Color term
 * used (3), then - as int32 bits - the ONE row that owns each minimum on this rank (3; the lowest tied row, as torch.min; -1 where the global minimum
 * lives on another rank): the backward hands the minimum's gradient to that row only; then d term / d alpha and d term / d scale per channel of both
 * loss objects (8; zeros without the adaptive loss).  Values are reduced without floating-point atomics, block sums in a fixed
 * order: two calls on the same inputs give the same bits.  d_scratch: snerf_loss_all_scratch_bytes() bytes, no initial state needed, one per stream.
 * backward: from d_g_vals (dL / d vals) to the gradients of snerf_loss_grads (what snerf_trainer_backward_image / _solar take); terms that are values
 * only contribute nothing, the gradient of a detached input is written as zeros; outputs of inputs the configuration lacks may be NULL. */
#define SNERF_LOSS_ADAPTIVE 1
#define SNERF_LOSS_PRIOR 2
#define SNERF_LOSS_SKY_DETACHED 4
typedef struct snerf_loss_in {
    int64_t n_rays, n_solar_rays;
    int n_samples, flags;
    const float *d_rgb, *d_rgb_merged, *d_gt, *d_albedo, *d_sky;           /* [n_rays,3]; d_rgb_merged optional */
    const float *d_solar_vis, *d_pv_exact, *d_pe_solar;                    /* sun-ray pass [n_solar_rays, n_samples] */
    const float *d_pe, *d_pe_supervised;                                   /* prior: image rays [n_rays, n_samples] */
    const float *d_alpha_color, *d_scale_color;                            /* adaptive: [3] */
    const float *d_alpha_alpha, *d_scale_alpha;                            /* adaptive + prior: [1] */
    const double *d_logz_value, *d_logz_slope;                             /* adaptive: [513], float64 */
    const float* d_albedo_min_global;                                      /* optional [3] + world: data parallel */
    int world;
    float w_solar, w_color, w_alpha;
} snerf_loss_in;
typedef struct snerf_loss_grads {
    float *d_g_rgb, *d_g_rgb_merged, *d_g_albedo, *d_g_sky;                /* [n_rays,3] */
    float *d_g_solar_vis;                                                  /* [n_solar_rays, n_samples] */
    float *d_g_pe;                                                         /* [n_rays, n_samples] */
    float *d_g_alpha_color, *d_g_scale_color, *d_g_alpha_alpha, *d_g_scale_alpha;
} snerf_loss_grads;
size_t snerf_loss_all_scratch_bytes(void);
int snerf_loss_all_term_count(int flags);
int snerf_loss_all_forward(const snerf_loss_in* in, void* d_scratch, float* d_vals, float* d_weights, float* d_aux14, void* stream);
int snerf_loss_all_backward(const snerf_loss_in* in, const float* d_aux14, const float* d_g_vals, const snerf_loss_grads* out, void* stream);
/* the same update (torch.optim.Adam, mg_run_NeRF.py:312-320) on caller-owned flat arenas of n floats */
int snerf_adam_step(float* d_params, const float* d_grads, float* d_m, float* d_v, int64_t n, float lr, float beta1, float beta2,
                    float eps, int step, void* stream);

/* ---- ray table on the GPU: P_img_Pinhole.invert_P (pre_NeRF/P_Img.py:133-147) over the pixel grid of
 * mg_Pt_holder.setup_quick_loader (mg_Pt_holder.py:178-194).  P_3x4: HOST pointer to the row-major 3x4 projective
 * camera (12 doubles).  Pixel (i, j) of the rows x cols grid is image pixel (i*downscale, j*downscale).  Writes
 * d_rows [rows*cols, 11] = Img_Pt(2) | Top(3, z=+1) | Bot(3, z=-1) | View(3) - the first 11 of the 22 training-row
 * columns (mg_run_NeRF.py:122-133; sun, time, weight, colour are per-image constants / image data) - and
 * d_valid [rows*cols] = 1 where Top and Bot lie inside [-1,1]^2 (the reference drops the others). */
int snerf_rays_from_camera(const double* P_3x4, int rows, int cols, int downscale, float* d_rows, uint8_t* d_valid, void* stream);

/* ---- novel-view ray grids on the GPU (the float64 numpy arithmetic of the reference, rounded to fp32 at its casts: bit-identical rays).
 * mode 0: component_render_by_dir (T_NeRF_Eval_Utils/mg_Img_Eval.py:96-115): grid rows linspace(1,-1,rows) (cube x), columns linspace(-1,1,cols)
 *         (cube y), z = 0; Top = grid + q, Bot = grid - q with params = q = v / v_z (3 doubles); no culling (d_valid: all 1).
 * mode 1: Quick_Run_Net._get_input_dict (T_NeRF_Full_2/Quick_Run.py:77-109): mids = XY * 2 / (size - 1) - 1 [remapped onto params[3..6] = region
 *         (x0, x1, y0, y1) when n_params == 7], Top / Bot = mids +- q; d_valid = 1 where Top and Bot lie in [-1,1]^3 (:95).
 * mode 2: component_render_by_P (mg_Img_Eval.py:74-94): params = 3x4 camera (12, row-major) + source image rows, cols; output pixel (r, c) looks at
 *         source pixel round(linspace(0, img - 1, out)) (d_pixels [n, 2], optional), rays by invert_P (pre_NeRF/P_Img.py:133-147) at h = +1 / -1,
 *         d_valid = 1 where both ends lie in [-1,1]^2 (:84-85).
 * Rays lo .. hi-1 of the row-major rows x cols grid (a rank's tile of a sharded render); params: HOST pointer; d_top / d_bot [hi - lo, 3]. */
int snerf_ray_grid(int mode, int rows, int cols, int64_t lo, int64_t hi, const double* params, int n_params, float* d_top, float* d_bot, uint8_t* d_valid,
                   int32_t* d_pixels, void* stream);

/* ---- DSM prior and validation helpers: the gathers the reference runs on the CPU between passes.
 * snerf_prior_density = T_NeRF.Supervised_Sample (T_NeRF_net_v2.py:175-181): rho = -log(1 - min(HM[ix,iy] >= z, .99)) / delta
 *   with (ix,iy) = trunc((xy+1)/2 * (shape-1)); d_height_map is the float64 [rows,cols] array the module is built with.
 *   d_outside (optional, [n]) supplies the value for points outside [-1,1]^3 (eval_Rho_Only keeps the network's own
 *   density there, Eval_Tools_2.py:321-326); with NULL every point must lie inside the cube.
 * snerf_surface_distance = Net_tool.get_Dist for one DSM (mg_run_NeRF.py:106-120): the expected distance along each ray
 *   to the first cell of the dense occupancy volume (DSM >= linspace(-1,1,S)[k], NaN cells kept: mg_run_NeRF.py:55-61);
 *   d_levels is that linspace in float64, d_tvals the eval-mode sample parameters; float64 [R] out (NaN = no surface).
 * snerf_image_error = the colour error sums of eval_img (mg_run_NeRF.py:204-208), accumulated into d_sums[3]:
 *   sum log(1/2 (gt-img)^2 + 1), sum (gt-img)^2, 3 * #pixels with any(gt != 0).  The caller zeroes d_sums. */
int snerf_prior_density(int64_t n_points, const float* d_points, const float* d_delta, const double* d_height_map,
                        int hm_rows, int hm_cols, const float* d_outside, float* d_rho_prior, void* stream);
int snerf_surface_distance(int64_t n_rays, int n_samples, const float* d_top, const float* d_bot, const float* d_tvals,
                           const double* d_dsm, int dsm_rows, int dsm_cols, const double* d_levels, double* d_dist,
                           void* stream);
int snerf_image_error(int64_t n_pixels, const float* d_image, const float* d_gt, double* d_sums, void* stream);
/* Eval_Tools_2.get_PV (Eval_Tools_2.py:13-16) as a stand-alone op: PV[r,s] = exp(-sum_{j<s} rho[r,j] * delta[r,j]) for
 * [n_rays, n_samples] arrays with arbitrary per-sample deltas (snerf_composite_rays fuses the same scan with the shading). */
int snerf_transmittance(int64_t n_rays, int n_samples, const float* d_rho, const float* d_delta, float* d_pv, void* stream);

/* ---- device ray loader: the reference's per-step data path - two DataLoader(shuffle=True, num_workers=4) collating batch_size single-row
 * __getitem__ calls (mg_run_NeRF.py:74-84, NN_loaders/mg_Color_Loader.py:94-102), Net_tool.get_data / data_to_dict (mg_run_NeRF.py:229-264, :122-133)
 * and SC_loader.__getitem__'s t.rand(4) per sun-check ray (NN_loaders/mg_SC_loader.py:17-21) - over a ray table that already lives on the device
 * (d_table [n_rows, 22] fp32: Img_Pt 2 | Top 3 | Bot 3 | View_Angle 3 | Sun_Angle 3 | Time_Encoded 4 | Sample_Weight 1 | GT_Color 3; owned by the
 * caller, alive as long as the loader).
 *   Shuffle without replacement: row i of a batch is table[perm_epoch(((batch_in_epoch * world) + rank) * batch + i)]; perm is a keyed bijection of
 *   [0, n_rows) - a balanced Feistel network over 2^k >= n_rows (k even), six rounds of murmur3's 32-bit finaliser, round keys from (seed, epoch),
 *   cycle-walking while the value is >= n_rows.  Exact integer arithmetic: snerf_loader_indices_host gives the same indices without a GPU.
 *   Epochs as DataLoader(shuffle=True): drop_last = 0 (the reference's default) ceil(n_rows / batch) batches, the last one short; drop_last = 1
 *   floor(n_rows / batch); world > 1 (data parallel) needs drop_last - floor(n_rows / (batch * world)) batches per epoch, the ranks taking disjoint
 *   consecutive batch-sized blocks of the ONE permutation.
 *   Sun-check rays: Philox4x32-10, key = the seed's (low, high) halves, counter = (i, draws low, draws high, rank), u = (word >> 8) * 2^-24;
 *   top = (u0 * dx + x0, u1 * dy + y0, z_hi), bot = (u2 * dx + x0, u3 * dy + y0, z_lo), product and sum rounded separately as torch's fp32 ops do;
 *   bounds6 (HOST, optional) = x0, x1, y0, y1, z_lo, z_hi (NULL: the cube [-1, 1]^3, setup_SC_loader's default), dx = x1 - x0 in fp32.
 *   State: four int64 in DEVICE memory {epoch, batch_in_epoch, draws, reserved}.  The kernels read the position from there, never from a launch
 *   argument, and a one-thread kernel behind the draw advances it: captured in a hipGraph (two kernel nodes), snerf_loader_next draws a new batch at
 *   every replay.  The handle keeps a host shadow, advanced by the same rule per (uncaptured) launch and used only to size a short last batch; a
 *   capture is refused (SNERF_E_STATE) unless every batch of an epoch has `batch` rows.  After replays the device copy is the truth
 *   (snerf_loader_get_state).
 * snerf_loader_create: SNERF_E_INVALID - before anything touches the GPU - for a NULL table, row_width != 22, n_rows < 1, batch < 1 (or >= 2^31),
 *   rank outside [0, world), world > 1 without drop_last, batch * world > n_rows with drop_last.
 * snerf_loader_next: every output is optional (NULL = skip); returns the row count of this batch (>= 1) or a negative SNERF_E_* code.
 * snerf_loader_set_state / _get_state: state4 is a HOST array; set writes both copies; both synchronise `stream` and are refused while it captures. */
typedef struct snerf_loader snerf_loader;
typedef struct snerf_loader_out {
    float* d_img_pt;        /* [B,2] */
    float* d_top;           /* [B,3] */
    float* d_bot;           /* [B,3] */
    float* d_view_angle;    /* [B,3] */
    float* d_sun_angle;     /* [B,3] */
    float* d_time_encoded;  /* [B,4] */
    float* d_sample_weight; /* [B,1] */
    float* d_gt_color;      /* [B,3] */
    int64_t* d_row_index;   /* [B] */
    float* d_sc_top;        /* [B,3] */
    float* d_sc_bot;        /* [B,3] */
} snerf_loader_out;
int snerf_loader_create(const float* d_table, int64_t n_rows, int row_width, int64_t batch, uint64_t seed, int drop_last, int rank, int world,
                        const float* bounds6, snerf_loader** out);
void snerf_loader_destroy(snerf_loader* l);
int64_t snerf_loader_batches_per_epoch(const snerf_loader* l);
int64_t snerf_loader_batch(const snerf_loader* l);       /* rows of a full batch: what every output buffer must hold */
int64_t snerf_loader_next(snerf_loader* l, const snerf_loader_out* out, void* stream);
int snerf_loader_get_state(snerf_loader* l, int64_t* state4, void* stream);
int snerf_loader_set_state(snerf_loader* l, const int64_t* state4, void* stream);
/* Host-only mirrors (no GPU): positions first .. first + count - 1 of epoch `epoch`'s permutation of [0, n_rows); the sun-check rays
 * first .. first + count - 1 of draw `draws` on `rank` (top / bot: [count, 3]).  snerf_loader_philox_host is the generator itself (counter 4 words,
 * key 2 words -> 4 words), for its known-answer vectors. */
int snerf_loader_indices_host(int64_t n_rows, uint64_t seed, int64_t epoch, int64_t first, int64_t count, int64_t* out);
int snerf_loader_sc_rays_host(uint64_t seed, int64_t draws, int rank, int64_t first, int64_t count, const float* bounds6, float* top, float* bot);
int snerf_loader_philox_host(const uint32_t* counter4, const uint32_t* key2, uint32_t* out4);

/* ---- per-step training inputs: what a training step draws besides its batch, on the device - the random sun rays of the solar-correction loss
 * (create_solor_rays_uniform, Eval_Tools_2.py:72-108), the jitter of both sampling passes (misc.sample_pt_coarse, misc.py:236-241) and one row of a
 * schedule table (Adam's six scalars, the DSM prior's trust factor, the second optimiser's learning rate).  Same law as the host draws, not the same
 * numbers: the stream is Philox4x32-10 keyed with the two halves of splitmix64(seed ^ 0x73746570696e7031) - distinct from the loader's sun-check words.
 *   Counter (index, draws low, draws high, rank + (block << 24)), rank < 2^24.
 *     block 0, index = ray i:     w0 azimuth, w1 elevation (u = w * 2^-32 in float64: az = u * 360 - 180, el = u * 89 + 1),
 *                                 w2 / w3 start x / y (u = (w >> 8) * 2^-24 in fp32: 2 * u - 1, product and sum rounded separately), start z = 1
 *     block 1, index = ray i:     w0 / w1 the two time angles (fp32 u * fp32(2 pi); cos / sin in float64 of that fp32 angle, rounded to fp32)
 *     block 2, index = sample s:  w0 / w1 jitter of the image / sun-ray pass: tv[s] = base[s] + fp32(1 / n_samples) * u, rounded separately
 *   vec = the world -> local direction of (el, az) in float64 (mg_unit_converter.py:5-9,59-68,29-34), written as fp32; ends = fp32(float64(starts) - 2 * vec / vec_z).
 *   Schedule: d_table [n_table_rows, 8] fp32 on the DEVICE (owned by the caller, alive as long as the handle); row `step` (past the end: the last row)
 *   goes to d_hyper (columns 0..5), d_trust (6), d_lr2 (7).
 *   State: four int64 in DEVICE memory {draws, step, reserved, reserved}, read by the draw kernel and advanced (+1, +1) by a one-thread kernel behind it:
 *   two kernel nodes in a hipGraph, a new draw at every replay.  The handle keeps a host shadow advanced per uncaptured launch.
 * snerf_step_inputs_create: SNERF_E_INVALID - before anything touches the GPU - for NULL pointers, n_rays < 1 or n_samples < 1 (or >= 2^31), rank outside
 *   [0, 2^24), a non-finite matrix or centre, n_table_rows < 1.  W2L_H (row-major 4x4) and world_center are HOST arrays.
 * snerf_step_inputs_draw: every output is optional (NULL = skip); the jitter outputs need d_base [n_samples] (linspace(0, 1, S + 1)[:-1]).
 * snerf_step_inputs_set_state / _get_state: state4 is a HOST array; both synchronise `stream` and are refused while it captures.
 * snerf_step_inputs_words_host (no GPU): the raw words of draw `draws` on `rank` - ray_words [n_rays, 8] (blocks 0 and 1), sample_words [n_samples, 4]. */
typedef struct snerf_step_inputs snerf_step_inputs;
typedef struct snerf_step_inputs_out {
    float* d_starts;        /* [R,3] */
    float* d_ends;          /* [R,3] */
    float* d_vec;           /* [R,3] */
    float* d_times;         /* [R,4] */
    const float* d_base;    /* [S] input */
    float* d_tv_image;      /* [S] */
    float* d_tv_solar;      /* [S] */
    float* d_hyper;         /* [6] */
    float* d_trust;         /* [1] */
    float* d_lr2;           /* [1] */
} snerf_step_inputs_out;
int snerf_step_inputs_create(uint64_t seed, int64_t n_rays, int64_t n_samples, int rank, const double* W2L_H, const double* world_center,
                             const float* d_table, int64_t n_table_rows, snerf_step_inputs** out);
void snerf_step_inputs_destroy(snerf_step_inputs* h);
int64_t snerf_step_inputs_rays(const snerf_step_inputs* h);          /* n_rays, n_samples, n_table_rows of the handle: what the outputs must hold */
int64_t snerf_step_inputs_samples(const snerf_step_inputs* h);
int64_t snerf_step_inputs_table_rows(const snerf_step_inputs* h);
int snerf_step_inputs_draw(snerf_step_inputs* h, const snerf_step_inputs_out* out, void* stream);
int snerf_step_inputs_get_state(snerf_step_inputs* h, int64_t* state4, void* stream);
int snerf_step_inputs_set_state(snerf_step_inputs* h, const int64_t* state4, void* stream);
int snerf_step_inputs_words_host(uint64_t seed, int64_t draws, int rank, int64_t n_rays, int64_t n_samples, uint32_t* ray_words, uint32_t* sample_words);

/* Name and launch geometry of the dominant kernel (for profiling scripts): fills grid/block/lds bytes. */
int snerf_field_kernel_info(const snerf_model* m, int64_t n_points, int* grid, int* block, int* lds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SEASON_NERF_HIP_H */
