// Kernel argument blocks and launch entry points (internal; the public surface is include/season_nerf_hip.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace snerf {

struct snerf_field_out_dev {
    float* rho;
    float* solar_vis;
    float* col_raw;
    float* adjust;
    float* col;
    float* adjust_col;
    float* points;
    float* vis;               // VARIANT 3 only: [n_rays] exp(-sum_{j < S-1} rho_j delta_j), one value per ray
};

constexpr int kVoteBytes = 64;    // LDS behind every fused kernel's image: one float per wave for the ray-visibility early-out vote (mlp_device.h raysum_saturated)

struct MlpArgs {
    const uint8_t* stream;     // packed fragment stream (device)
    uint32_t stream_bytes;     // bytes consumed per tile = length of the cyclic DMA stream
    const float* bias;         // bias table (device)
    int bias_floats;
    int64_t n;                 // points (field program) or groups (group program)
    int n_classes;
    // field program inputs
    const float* points;       // [n,3] or NULL -> generate from rays
    const float* top;          // [R,3]
    const float* bot;          // [R,3]
    const float* tvals;        // [S]
    int n_samples;
    int64_t group_size;        // points per sun/classes row
    const float* sun;          // [G,3]
    const float* classes;      // [G,C] or NULL
    snerf_field_out_dev out;
    // group program inputs / outputs
    const float* time;         // [G,4]
    float* g_classes;          // [G,C]
    float* g_sky_raw;          // [G,3]
    float* g_sky;              // [G,3]
    uint32_t debug;            // only read by -DSNERF_ABLATE builds
    // VARIANT 3 (ray visibility: the density-only program with the sum over a ray's samples kept in registers): n = rays, every wave
    // owns one ray of a group of `waves per workgroup` rays and walks its samples 32 at a time
    int k64;                   // mlp_i8x2_kernel: stream and tables are in the 16x16x64 layout (program.h "k64"); 0 everywhere else
    int ray_flags;             // bit 1: a sample outside [-1,1]^3 contributes nothing (mg_Img_Eval.py:42,65-66); bit 2: no early-out (A/B); bit 3: passes from the sun side inwards (the order before round 6's reversal, A/B)
};

// Sun walk (sun_walk_kernel / sun_walk_ks_kernel): the variant-0 layer walk with fc_solar_1..4 repeated for n_suns sun directions.  Wraps MlpArgs
// so that the argument layout of the existing kernels stays as it is.  m.sun is [n_suns,3], m.out.solar_vis [n_suns, m.n]; m.stream is the walk
// stream (program.h sun_walk_*) and m.stream_bytes its whole length.
constexpr int kMaxWalkSuns = 32;
struct SunWalkArgs {
    MlpArgs m;
    int n_suns;
};

// Ray surface (ray_surface_kernel / ray_surface_ks_kernel, mlp_device.h RaySurf): the density-only walk of VARIANT 3 with the compositing scan inside.
// Wraps MlpArgs as SunWalkArgs does.  m.n = rays, m.stream = the field stream cycled over the layers of variant 3, m.ray_flags bit 3 always set
// (passes from t = 0 downwards); out [n,4] = {sum PS, sum PS t, sum PS s, optical depth walked} per ray, 16-byte aligned.
struct RaySurfaceArgs {
    MlpArgs m;
    float* out;
};

// Shadow walk (shadow_walk_kernel / shadow_walk_ks_kernel, mlp_device.h RayShadow): the ray surface's walk through the layers of variant 1 with the
// reference's shadow test inside.  m as in RaySurfaceArgs, with m.stream = the field stream cycled over the layers of variant 1; sun [n,3] = one sun
// direction per ray, as the caller gives it; out [n,8] = {n(PV > .5 and vis > .5), n(PV > .5), n(vis > .5), sum (PV - vis)^2, sum |PV - vis|, sum PS vis,
// sum PS, optical depth walked} per ray, 32-byte aligned.
struct ShadowWalkArgs {
    MlpArgs m;
    const float* sun;
    float* out;
};

// Film frame (frame_walk_kernel / frame_walk_ks_kernel, mlp_device.h RayFrame): the ray surface's walk through the layers of variant 0 with the shading and
// compositing of the reference's film frames inside.  m as in RaySurfaceArgs, with m.stream = the unchanged variant-0 field stream.  The same for every ray:
// sun [3], sky [3] (sigmoided), class_vecs [n_times, m.n_classes] with 1 <= n_times <= kMaxFrameTimes, delta.  out [n,16] = {rgb of season k at 3k..3k+2
// (0 for k >= n_times), [12] sum PS, [13] sum PS s, [14] optical depth walked, [15] sum PS vis} per ray, 64-byte aligned.
constexpr int kMaxFrameTimes = 4;
struct FrameWalkArgs {
    MlpArgs m;
    const float* sun;
    const float* sky;
    const float* class_vecs;
    int n_times;
    float delta;
    float* out;
};

// Solar audit (solar_audit_kernel / solar_audit_ks_kernel, mlp_device.h RayAudit): the density-only walk of variant 3 along the secondary rays of the samples of
// primary rays, formed in the kernel, scored against the learned visibility.  m as in RaySurfaceArgs (m.n = PRIMARY rays, m.top / m.bot theirs), m.ray_flags
// without bit 3 (passes from the point outwards); sun = the sun direction in float64, by value; est_vis, ps [n, S]; out [n,8] = {n(E > .5 and V > .5),
// n(E > .5), n(V > .5), sum E PS, sum V PS, sum PS, sum (E - V)^2, sum |E - V|} per primary ray, 32-byte aligned; exact [n, S] or NULL = E per sample.
struct SolarAuditArgs {
    MlpArgs m;
    double sun[3];
    const float* est_vis;
    const float* ps;
    float* out;
    float* exact;
};

struct CompOutDev {
    float *rgb, *albedo, *pv, *pe, *ps, *delta, *shadow, *acc, *surf_loc, *surf_dist;
};

struct CompArgs {
    int64_t n_rays;
    int n_samples;
    const float *top, *bot, *tvals;
    const float *rho, *col, *solar_vis, *sky;
    int flags;
    const float* rho_prior;
    float trust;
    const float* trust_dev;       // optional: the trust factor read from device memory at run time (captured steps); overrides `trust`
    CompOutDev out;
};

struct RayGenArgs {
    double P[12];          // row-major 3x4, normalised so that P[11] = 1 is NOT assumed
    int rows, cols, ds;
    float* rows_out;       // [rows*cols, 11]: img_pt 2 | top 3 | bot 3 | view 3
    uint8_t* valid;        // [rows*cols] or NULL
};
hipError_t launch_rays_from_camera(const RayGenArgs& a, hipStream_t st);

// novel-view ray grids (float64 arithmetic as the reference's numpy, rounded to fp32 at the end)
struct RayGridArgs {
    int mode;              // 0: by direction (mg_Img_Eval.py:96-115), 1: Quick_Run (Quick_Run.py:77-109), 2: through a 3x4 camera (mg_Img_Eval.py:74-94)
    int rows, cols;        // the output grid H x W
    int64_t lo, hi;        // rays lo .. hi-1 of the row-major grid
    double q[3];           // modes 0, 1: view vector / its z component
    int has_region;        // mode 1
    double region[4];
    double P[12];          // mode 2
    int img_rows, img_cols;
    float *top, *bot;      // [hi - lo, 3]
    uint8_t* valid;        // [hi - lo] or NULL
    int32_t* pix;          // mode 2, optional: [hi - lo, 2] source pixel (row, col)
};
hipError_t launch_ray_grid(const RayGridArgs& a, hipStream_t st);

struct SweepArgs {
    int64_t n_rays;
    int n_samples, n_classes, n_times, flags;
    const float *top, *bot, *tvals;
    const float* deltas;       // optional [R,S]: explicit segment lengths (then top / bot / tvals are not read)
    const float *rho, *col_raw, *adjust, *solar_vis;
    int adjust_vec4;           // adjust is 16-byte aligned and n_classes == 4: a sample's 12 values are three 16-byte loads
    const float* sky;          // [3]
    const float* class_vecs;   // [T,C]
    float *season, *shaded;    // [T,R,3]
    float* classic;            // optional [T,R,3]: sum_s PS * sigmoid(.) * (SV + (1-SV)*sky)  (mg_Img_Eval.py:165-170)
    float *base, *shadow_adjust, *raw_shadow;   // [R,3], [R,3], [R]
};
hipError_t launch_sweep(const SweepArgs& a, hipStream_t st);
// grid compositing of a sun walk (sun_walk_composite_kernel): the sweep's season images times the shadow factors of n_suns sun directions
struct SunWalkCompArgs {
    int64_t n_rays;
    int n_samples, n_classes, n_times, n_suns, flags;
    const float *top, *bot, *tvals;
    const float* deltas;       // optional [R,S], as SweepArgs
    const float *rho, *col_raw, *adjust;
    const float* solar_vis;    // [M,R,S]
    const float* sky;          // [M,3]
    const float* class_vecs;   // [T,C]
    float* shaded;             // [M,T,R,3]
    float* season;             // [T,R,3]
    float* base;               // [R,3]
    float* raw_shadow;         // [M,R]
    float* shadow_adjust;      // [M,R,3]
};
int sun_walk_composite_lds_bytes(int n_samples, int n_suns);
hipError_t launch_sun_walk_composite(const SunWalkCompArgs& a, hipStream_t st);
// workgroup tiles of a fused field launch: `rays` rays per tile in VARIANT 3 (ray visibility), `pts` points per tile otherwise
__host__ __device__ inline int64_t field_tiles(int64_t n, int variant, int pts, int rays) { return variant == 3 ? (n + rays - 1) / rays : (n + pts - 1) / pts; }
hipError_t launch_mlp(int prog, int W, int variant, bool fast, const MlpArgs& a, int n_cu, hipStream_t st);
hipError_t launch_ray_surface(int W, const RaySurfaceArgs& a, int n_cu, hipStream_t st);                    // kernels.hip (W = 64, 256), kernels_ks.hip (W = 512)
hipError_t launch_ray_surface_ks(int W, const RaySurfaceArgs& a, int n_cu, hipStream_t st);
hipError_t launch_shadow_walk(int W, const ShadowWalkArgs& a, int n_cu, hipStream_t st);                    // kernels.hip (W = 64, 256), kernels_ks.hip (W = 512)
hipError_t launch_shadow_walk_ks(int W, const ShadowWalkArgs& a, int n_cu, hipStream_t st);
hipError_t launch_frame_walk(int W, const FrameWalkArgs& a, int n_cu, hipStream_t st);                      // kernels.hip (W = 64, 256), kernels_ks.hip (W = 512)
hipError_t launch_frame_walk_ks(int W, const FrameWalkArgs& a, int n_cu, hipStream_t st);
hipError_t launch_solar_audit(int W, const SolarAuditArgs& a, int n_cu, hipStream_t st);                    // kernels.hip (W = 64, 256), kernels_ks.hip (W = 512)
hipError_t launch_solar_audit_ks(int W, const SolarAuditArgs& a, int n_cu, hipStream_t st);
hipError_t launch_sun_walk(int W, const SunWalkArgs& a, int n_cu, hipStream_t st);                          // kernels.hip (W = 64, 256), kernels_ks.hip (W = 512)
hipError_t launch_sun_walk_ks(int W, const SunWalkArgs& a, int n_cu, hipStream_t st);
hipError_t launch_mlp_i8(int W, int variant, const MlpArgs& a, int n_cu, hipStream_t st);                // kernels_i8.hip (field program only)
int field_variant_chunks_i8(int W, int C, int variant);
hipError_t launch_mlp_i8x2(int W, int variant, const MlpArgs& a, int n_cu, hipStream_t st);                // kernels_i8x2.hip (W <= 256)
bool i8x2_k64_built(int W, int variant);                                                                   // ... is this instance built on v_mfma_i32_16x16x64_i8 (and reads the k64 stream)?
hipError_t launch_mlp_ks(int W, int variant, const MlpArgs& a, int n_cu, hipStream_t st);                // kernels_ks.hip (W = 512, bf16x3, K split over wave pairs)
hipError_t launch_mlp_ks_group(int W, const MlpArgs& a, int n_cu, hipStream_t st);                         // ... its per-ray (time / sun) networks
hipError_t launch_mlp_group_split(int W, const MlpArgs& a, int n_cu, hipStream_t st);                   // kernels_group.hip (W <= 256: the per-ray networks, output blocks split over the waves)
int field_variant_chunks_ks(int W, int C, int variant);
int group_chunks_ks(int W, int C);
int mlp_ks_lds_bytes(int bias_floats);
int mlp_ks_tile_points();
hipError_t launch_composite(const CompArgs& a, hipStream_t st);
// dsm.hip
hipError_t launch_prior_density(int64_t n, const float* pts, const float* delta, const double* hm, int hx, int hy, const float* outside,
                                float neg_log_term, float* rho, hipStream_t st);
hipError_t launch_surface_distance(int64_t n_rays, int S, const float* top, const float* bot, const float* tvals, const double* dsm, int dx,
                                   int dy, const double* levels, double* dist, hipStream_t st);
hipError_t launch_image_error(int64_t n_pix, const float* img, const float* gt, double* sums, hipStream_t st);
hipError_t launch_transmittance(int64_t n_rays, int S, const float* rho, const float* delta, float* pv, hipStream_t st);
// loader.hip: one training batch drawn from the device-resident ray table; the position (epoch, batch) is read from d_state, not from an argument
struct LoaderArgs {
    const float* table;        // [n_rows, 22]
    int64_t n_rows, batch;     // batch = B of the position formula p = ((batch_in_epoch * world) + rank) * B + i
    int64_t rows;              // rows this launch writes (< batch only in a short last batch)
    int64_t batches_per_epoch;
    const int64_t* state;      // {epoch, batch_in_epoch, draws, reserved}
    uint64_t seed;
    int rank, world, bits;
    float *img_pt, *top, *bot, *view, *sun, *time, *weight, *gt;     // each optional
    int64_t* index;            // optional [rows]
    float *sc_top, *sc_bot;    // optional [rows, 3]
    float x0, dx, y0, dy, z_lo, z_hi;
};
hipError_t launch_loader_draw(const LoaderArgs& a, hipStream_t st);
hipError_t launch_loader_advance(int64_t* state, int64_t batches_per_epoch, hipStream_t st);
// loader.hip: what a training step draws per step besides its batch - random sun rays, both jitter vectors, one row of the schedule table
struct StepInputsArgs {
    const int64_t* state;      // {draws, step, reserved, reserved}
    uint64_t seed;
    uint32_t rank;
    int64_t n_rays, n_samples;
    double H[12];              // rows 0..2 of the world -> local matrix
    double wc[3];              // world centre (lat, lon, height)
    double lon_scale;          // 1000 * R_km * cos(deg2rad(lat)) of the centre
    float inv_s;               // fp32(1 / n_samples)
    const float* base;         // [n_samples]: linspace(0, 1, S + 1)[:-1]; needed with tv_image / tv_solar
    const float* table;        // [table_rows, 8]
    int64_t table_rows;
    float *starts, *ends, *vec, *times;      // each optional: [n_rays, 3] x 3, [n_rays, 4]
    float *tv_image, *tv_solar;              // each optional: [n_samples]
    float *hyper, *trust, *lr2;              // each optional: [6], [1], [1]
};
hipError_t launch_step_inputs_draw(const StepInputsArgs& a, hipStream_t st);
hipError_t launch_step_inputs_advance(int64_t* state, hipStream_t st);
int mlp_lds_bytes(int bias_floats);
int mlp_tile_points();
int field_variant_chunks(int W, int C, int variant);
const char* mlp_kernel_name();

}  // namespace snerf
