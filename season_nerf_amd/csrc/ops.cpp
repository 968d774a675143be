// PyTorch-ROCm custom-op layer over the C ABI (include/season_nerf_hip.h): TORCH_LIBRARY(season_nerf, m).
//
// The reference has no operator registry (pure PyTorch); these are the ops its Python seams call in this
// build: every op takes / returns at::Tensor, validates with TORCH_CHECK (-> RuntimeError), runs on the current HIP
// stream of the tensors' device, allocates its outputs with the caching allocator (PyTorch owns all memory, the
// kernels own nothing) and is visible to the dispatcher, the profiler and torch.library.opcheck.  The arithmetic is
// in libseason_nerf_hip.so; nothing here computes.
//
//   torch.classes.season_nerf.Model(W, C, precision)      T_NeRF(layer_width, n_classes) packed weights  (T_NeRF_net_v2.py:20-60)
//     .set_tensor(key, cpu_f32)  .resolve()  .i8_estimate()  .finalize()  .width()  .classes()  .precision()  .handle()
//   season_nerf::group_fwd(Model, time[G,4], sun[G,3]) -> (classes[G,C], sky_raw[G,3], sky[G,3])        get_class_only + sky head
//   season_nerf::points_fwd(Model, x[N,3], sun[G,3]?, classes[G,C]?, group_size, variant)               T_NeRF.forward* on points
//   season_nerf::ray_visibility(Model, top[R,3], bot[R,3], tvals[S], flags) -> vis[R]                     exact solar visibility of secondary rays
//        -> (rho[N,1], solar_vis[N,1], col_raw[N,3], adjust[N,C,3], col[N,3], adjust_col[N,3])
//   season_nerf::render_fwd(Model, top[R,3], bot[R,3], sun[R,3], time[R,4], tvals[S], flags, want_per_sample, want_unmixed=False)
//        -> (rgb[R,3], depth[R,2] = (surface distance, accumulated weight), albedo[R,3], per_sample[])  All_in_One_Eval.eval
//   season_nerf::composite(top, bot, tvals, rho, col, solar_vis, sky, flags, rho_prior?, trust) -> Tensor[10]    get_PV + shading
//   season_nerf::composite_sweep(...) -> Tensor[6]                                                    mg_Img_Eval t-step sweep
//   season_nerf::sun_walk_fwd(model, top[R,3], bot[R,3], tvals[S], suns[M,3], classes[C]?)             one field pass, M sun directions
//        -> [rho[R,S,1], solar_vis[M,R,S,1], col_raw[R,S,3], adjust[R,S,C,3], points[R,S,3]]             (mg_Season_Eval.py:74-98; `model` = Model.handle())
//   season_nerf::composite_sun_walk(top, bot, tvals, rho, col_raw, adjust, solar_vis[M,R,S], sky[M,3], class_vecs[T,C], flags, deltas?)
//        -> [shaded[M,T,R,3], season[T,R,3], base[R,3], raw_shadow[M,R], shadow_adjust[M,R,3]]           the M x T grid of a view
//   season_nerf::ray_surface(model, top[R,3], bot[R,3], tvals[S], flags) -> [R,4] {sum PS, sum PS t, sum PS s, optical depth}      height maps from a density-only ray pass
//   season_nerf::shadow_walk(model, top[R,3], bot[R,3], sun[R,3], tvals[S], flags) -> [R,8]           the shadow test's per-ray sums (mg_Shadow_Eval.py:72-104,134-163)
//   season_nerf::solar_audit(model, top[R,3], bot[R,3], tvals[S], sun (3 float64), est_vis[R,S], ps[R,S], flags, want_exact) -> ([R,8], [R,S] or [0,0])   the solar audit's per-ray sums, Exact_Solar (mg_Advanced_Solar.py)
//   season_nerf::frame_walk(model, top[R,3], bot[R,3], tvals[S], delta, sun[3], sky[3], class_vecs[T,C], flags) -> [R,16]   a film frame's per-ray sums, T <= 4 seasons (mg_movie_maker.py:108-187)
//   season_nerf::fused_adam_(param!, grad, m!, v!, lr, b1, b2, eps, step) -> ()                         mg_run_NeRF.py:312-320
// Training engine (csrc/train.cpp; `trainer` = the snerf_trainer handle a season_nerf_amd.training.TrainEngine owns and has bound to its
// parameter / gradient / workspace tensors).  The forward ops are functional in their tensor arguments (torch.library.register_autograd
// attaches the backward ops to them, season_nerf_amd/training.py); the engine keeps the activations of its last forward and the BatchNorm
// running statistics behind the handle.  `params` only ties the ops into the autograd graph of the parameters.
// train_bn = false (a module in .eval(): frozen BatchNorm, running statistics) is differentiable too: the engine remembers the mode of each pass's
// forward and train_bwd_image / train_bwd_points return the gradient of THAT function (dz = gamma istd dy through a frozen layer; the biases in front
// of BatchNorm get a gradient); nothing of the running statistics changes.
//   season_nerf::train_fwd_image(trainer, top, bot, tvals, sun, time, train_bn, classic, n_classes, height_map?, trust, trust_dev?, params[])       get_loss, image rays
//        -> [rgb, albedo, sky, pe, rgb_merged, albedo_merged | pv, ps, delta, classes, rho, solar_vis, col, pts, adjust_col | prior terms]  Eval_Tools_2.py:165-252
//   season_nerf::train_bwd_image(trainer, grads!, g_rgb?, g_albedo?, g_sky?, g_pe?, rho_prior?, trust, g_rgb_merged?, g_albedo_merged?) -> ()
//   season_nerf::train_fwd_points(trainer, x, sun, time, train_bn, n_classes, params[]) -> [rho, col, solar_vis, sky, classes, adjust_col, col_raw, adjust]
//   season_nerf::train_bwd_points(trainer, grads!, g_rho?, g_col?, g_solar_vis?, g_sky?, g_classes?) -> ()                                T_NeRF.forward, train mode
//   season_nerf::train_fwd_solar(trainer, top, bot, tvals, sun, train_bn, params[]) -> [solar_vis, pv, pe, sky_raw, rho, pts, delta]      eval_Rho_Only / forward_Solar
//   season_nerf::train_bwd_solar(trainer, grads!, g_solar_vis) -> ()
//   season_nerf::prior_density(pts[N,3], delta[N], height_map[h,w] f64, outside[N]?) -> rho_prior[N,1]                                    T_NeRF.Supervised_Sample
// Device ray loader (csrc/loader.hip; `loader` = the snerf_loader handle a season_nerf_amd.loader.DeviceRayLoader owns):
//   season_nerf::loader_next(loader, table[N,22], img_pt!?, top!?, bot!?, view_angle!?, sun_angle!?, time_encoded!?, sample_weight!?, gt_color!?, row_index!?,
//        sc_top!?, sc_bot!?) -> ()        the next shuffled batch written into the given buffers ([>= batch, w] each, None = skip); the position lives in
//        device memory behind the handle and advances per call - and per replay of a graph that captured the call            get_data, mg_run_NeRF.py:229-264
//   season_nerf::step_inputs_draw(handle, table[K,8], starts!?, ends!?, vec!?, times!?, base?, tv_image!?, tv_solar!?, hyper!?, trust!?, lr2!?) -> ()
//        the step's random sun rays, both jitter vectors and row `step` of the schedule table (`handle` = the snerf_step_inputs of a
//        season_nerf_amd.step_inputs.DeviceStepInputs); position in device memory as above                          Eval_Tools_2.py:72-108, misc.py:236-241
#include <ATen/ATen.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>      // PyTorch-ROCm presents HIP devices under the "cuda" device type
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>
#include <torch/custom_class.h>
#include <torch/library.h>

#include <string>
#include <tuple>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/season_nerf_hip.h"

namespace {

using at::Tensor;

void ck(int rc, const char* what) { TORCH_CHECK(rc == SNERF_OK, "season_nerf::", what, " failed (code ", rc, "): ", snerf_last_error()); }

const float* fptr(const Tensor& t) { return t.data_ptr<float>(); }
float* mptr(Tensor& t) { return t.data_ptr<float>(); }

void check_dev_f32(const Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda(), name, " must live on the GPU (got ", t.device(), ")");
    TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32 (got ", t.scalar_type(), ")");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
void check_shape(const Tensor& t, const char* name, int64_t rows, int64_t cols) {
    check_dev_f32(t, name);
    TORCH_CHECK(t.dim() == 2 && (rows < 0 || t.size(0) == rows) && t.size(1) == cols, name, " must be [", rows < 0 ? std::string("N") : std::to_string(rows), ",",
                cols, "], got ", t.sizes());
}
// the rays of an op: top, bot [R,3] and the sample positions tvals [S] with S >= min_samples, all float32 on the device -> (R, S)
std::pair<int64_t, int64_t> check_rays(const Tensor& top, const Tensor& bot, const Tensor& tvals, int64_t min_samples = 1) {
    check_shape(top, "top", -1, 3);
    check_shape(bot, "bot", top.size(0), 3);
    check_dev_f32(tvals, "tvals");
    TORCH_CHECK(tvals.dim() == 1 && tvals.numel() >= min_samples, min_samples > 1 ? "tvals must be [S] with S >= " : "tvals must be [S]",
                min_samples > 1 ? std::to_string(min_samples) : std::string());
    return {top.size(0), tvals.numel()};
}
void* cur_stream(const Tensor& t) { return (void*)c10::hip::getCurrentHIPStreamMasqueradingAsCUDA(t.device().index()).stream(); }

struct Model : torch::CustomClassHolder {
    snerf_model* m = nullptr;
    bool owner = true;
    Model(int64_t W, int64_t C, const std::string& precision) {
        m = snerf_model_create((int)W, (int)C);
        TORCH_CHECK(m, "season_nerf::Model: ", snerf_last_error());
        const int p = precision == "bf16x3" ? SNERF_PREC_BF16X3 : precision == "bf16" ? SNERF_PREC_BF16 : precision == "i8x3" ? SNERF_PREC_I8X3
                    : precision == "auto" ? SNERF_PREC_AUTO : -1;
        if (p < 0 || snerf_model_set_precision(m, p) != SNERF_OK) {
            snerf_model_destroy(m);
            m = nullptr;
            TORCH_CHECK(false, "season_nerf::Model: precision must be 'auto', 'bf16x3', 'bf16' or 'i8x3' (got '", precision, "')");
        }
    }
    Model(int64_t handle, bool) : m((snerf_model*)handle), owner(false) {}       // view of a model the ctypes binding owns
    ~Model() override {
        if (m && owner) snerf_model_destroy(m);
    }
    void set_tensor(const std::string& key, const Tensor& t) {
        TORCH_CHECK(t.device().is_cpu() && t.scalar_type() == at::kFloat, "set_tensor(", key, "): host float32 tensor expected");
        const Tensor c = t.contiguous();
        ck(snerf_model_set_tensor(m, key.c_str(), c.data_ptr<float>(), (size_t)c.numel()), "Model.set_tensor");
    }
    void finalize() { ck(snerf_model_finalize(m), "Model.finalize"); }
    int64_t width() const { return snerf_model_width(m); }
    int64_t classes() const { return snerf_model_classes(m); }
    int64_t precision() const { return snerf_model_precision(m); }
    // host-only: packs the weights and returns the mode the model runs in ('auto' resolved), or a negative SNERF_E_* code
    // (SNERF_E_INVALID: no fused kernel for the resolved mode at this width)
    int64_t resolve() { return snerf_model_resolve_precision(m); }
    // [density, colour, solar visibility, adjust | hidden | worst | rgb_pred | budget | accumulator bound | ok]
    std::vector<double> i8_estimate() {
        snerf_i8_estimate e;
        ck(snerf_model_i8_estimate(m, &e), "Model.i8_estimate");
        return {e.head_rms[0], e.head_rms[1], e.head_rms[2], e.head_rms[3], e.hidden_rms, e.worst, e.rgb_pred, e.budget,
                (double)e.acc_bound, (double)e.ok};
    }
    int64_t handle() const { return (int64_t)m; }
};
using ModelPtr = c10::intrusive_ptr<Model>;

c10::intrusive_ptr<Model> model_from_handle(int64_t handle) {
    TORCH_CHECK(handle != 0, "season_nerf::model_from_handle: NULL handle");
    return c10::make_intrusive<Model>(handle, false);
}

std::tuple<Tensor, Tensor, Tensor> group_fwd(const ModelPtr& M, const Tensor& time, const Tensor& sun) {
    check_shape(time, "time", -1, 4);
    check_shape(sun, "sun", time.size(0), 3);
    c10::hip::HIPGuardMasqueradingAsCUDA g(time.device());
    const int64_t G = time.size(0);
    Tensor cls = at::empty({G, M->classes()}, time.options()), sky_raw = at::empty({G, 3}, time.options()), sky = at::empty({G, 3}, time.options());
    ck(snerf_group_forward(M->m, G, fptr(time), fptr(sun), mptr(cls), mptr(sky_raw), mptr(sky), cur_stream(time)), "group_fwd");
    return {cls, sky_raw, sky};
}

std::vector<Tensor> points_fwd(const ModelPtr& M, const Tensor& x, const c10::optional<Tensor>& sun, const c10::optional<Tensor>& classes,
                               int64_t group_size, int64_t variant) {
    check_shape(x, "x", -1, 3);
    TORCH_CHECK(variant >= 0 && variant <= 2, "variant must be 0 (everything), 1 (density + solar visibility) or 2 (density)");
    TORCH_CHECK(group_size >= 1, "group_size must be >= 1");
    const int64_t N = x.size(0), C = M->classes(), G = (N + group_size - 1) / group_size;
    if (variant <= 1) {
        TORCH_CHECK(sun.has_value(), "sun directions are required for variants 0 and 1");
        check_shape(*sun, "sun", G, 3);
    }
    if (classes.has_value()) check_shape(*classes, "classes", G, C);
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    auto o = x.options();
    Tensor rho = at::empty({N, 1}, o), sv = at::empty({variant <= 1 ? N : 0, 1}, o), col_raw = at::empty({variant == 0 ? N : 0, 3}, o),
           adjust = at::empty({variant == 0 ? N : 0, C, 3}, o), col = at::empty({variant == 0 ? N : 0, 3}, o), adjc = at::empty({variant == 0 ? N : 0, 3}, o);
    snerf_field_out fo{};
    fo.d_rho = mptr(rho);
    if (variant <= 1) fo.d_solar_vis = mptr(sv);
    if (variant == 0) { fo.d_col_raw = mptr(col_raw); fo.d_adjust = mptr(adjust); fo.d_col = mptr(col); fo.d_adjust_col = mptr(adjc); }
    ck(snerf_field_forward_points(M->m, (int)variant, N, fptr(x), group_size, sun.has_value() ? fptr(*sun) : nullptr,
                                  classes.has_value() ? fptr(*classes) : nullptr, &fo, cur_stream(x)), "points_fwd");
    return {rho, sv, col_raw, adjust, col, adjc};
}

// exact solar visibility of secondary rays (Eval_Tools_2.py:255-271, mg_Img_Eval.py:57-70): one launch, one float per ray
Tensor ray_visibility(const ModelPtr& M, const Tensor& top, const Tensor& bot, const Tensor& tvals, int64_t flags) {
    const auto [R, S] = check_rays(top, bot, tvals);
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    Tensor vis = at::empty({R}, top.options());
    ck(snerf_field_ray_visibility(M->m, R, (int)S, fptr(top), fptr(bot), fptr(tvals), (int)flags, mptr(vis), cur_stream(top)), "ray_visibility");
    return vis;
}

std::tuple<Tensor, Tensor, Tensor, std::vector<Tensor>> render_fwd(const ModelPtr& M, const Tensor& top, const Tensor& bot, const Tensor& sun,
                                                                   const Tensor& time, const Tensor& tvals, int64_t flags, bool want_per_sample, bool want_unmixed) {
    const auto [R, S] = check_rays(top, bot, tvals);
    check_shape(sun, "sun", R, 3);
    check_shape(time, "time", R, 4);
    const int64_t C = M->classes();
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    auto o = top.options();
    Tensor rgb = at::empty({R, 3}, o), depth = at::empty({R, 2}, o), albedo = at::empty({R, 3}, o);
    Tensor dist = at::empty({R}, o), acc = at::empty({R}, o);
    Tensor ws = at::empty({(int64_t)snerf_render_workspace_bytes(R, (int)S, (int)C)}, o.dtype(at::kByte));
    std::vector<Tensor> per;
    snerf_field_out fo{};
    snerf_composite_out co{};
    co.d_albedo = mptr(albedo);
    co.d_surf_dist = mptr(dist);
    co.d_acc = mptr(acc);
    if (want_per_sample) {
        // Rho, Col, Solar_Vis, Adjust, Adjust_col, Col_raw, sample_pts, PV, PE, PS, deltas (the per-sample keys of eval's result
        // dict), then the per-ray Classes [R,C] and Sky_Col [R,3]
        // Adjust [R,S,C,3] and Col_raw (the unmixed seasonal terms: forward_seperate, the seasonal sweep) only on request: eval's result
        // dict does not carry them, and at 4096 x 96, C = 4 they are 23.6 MB of HBM writes - as much as everything else the kernel moves
        const int64_t U = want_unmixed ? R : 0;
        per = {at::empty({R, S, 1}, o), at::empty({R, S, 3}, o), at::empty({R, S, 1}, o), at::empty({U, S, C, 3}, o), at::empty({R, S, 3}, o),
               at::empty({U, S, 3}, o), at::empty({R, S, 3}, o), at::empty({R, S, 1}, o), at::empty({R, S, 1}, o), at::empty({R, S, 1}, o),
               at::empty({R, S, 1}, o)};
        fo.d_rho = mptr(per[0]); fo.d_col = mptr(per[1]); fo.d_solar_vis = mptr(per[2]); fo.d_adjust_col = mptr(per[4]);
        if (want_unmixed) { fo.d_adjust = mptr(per[3]); fo.d_col_raw = mptr(per[5]); }
        fo.d_points = mptr(per[6]);
        co.d_pv = mptr(per[7]); co.d_pe = mptr(per[8]); co.d_ps = mptr(per[9]); co.d_delta = mptr(per[10]);
    }
    ck(snerf_render_rays(M->m, R, (int)S, fptr(top), fptr(bot), fptr(tvals), fptr(sun), fptr(time), (int)flags, mptr(rgb), &fo, &co, ws.data_ptr(),
                         (size_t)ws.numel(), cur_stream(top)), "render_fwd");
    depth.select(1, 0).copy_(dist);
    depth.select(1, 1).copy_(acc);
    if (want_per_sample) {
        // per-ray season classes [R,C] and sky colour [R,3]: views of the workspace regions snerf_render_rays filled
        const int64_t a256 = 256, cls_b = (R * C * 4 + a256 - 1) / a256 * a256, r3_b = (R * 3 * 4 + a256 - 1) / a256 * a256;
        per.push_back(ws.narrow(0, 0, R * C * 4).view(at::kFloat).reshape({R, C}));
        per.push_back(ws.narrow(0, cls_b + r3_b, R * 3 * 4).view(at::kFloat).reshape({R, 3}));
    }
    return {rgb, depth, albedo, per};
}

std::vector<Tensor> composite(const Tensor& top, const Tensor& bot, const Tensor& tvals, const Tensor& rho, const Tensor& col, const Tensor& solar_vis,
                              const Tensor& sky, int64_t flags, const c10::optional<Tensor>& rho_prior, double trust) {
    check_shape(top, "top", -1, 3);
    const int64_t R = top.size(0);
    check_shape(bot, "bot", R, 3);
    check_dev_f32(tvals, "tvals");
    const int64_t S = tvals.numel();
    check_dev_f32(rho, "rho"); check_dev_f32(col, "col"); check_dev_f32(solar_vis, "solar_vis");
    TORCH_CHECK(rho.numel() == R * S && solar_vis.numel() == R * S && col.numel() == R * S * 3, "rho / solar_vis / col must hold R*S (x3) elements");
    check_shape(sky, "sky", R, 3);
    if (rho_prior.has_value()) { check_dev_f32(*rho_prior, "rho_prior"); TORCH_CHECK(rho_prior->numel() == R * S, "rho_prior must hold R*S elements"); }
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    auto o = top.options();
    std::vector<Tensor> r = {at::empty({R, 3}, o), at::empty({R, 3}, o), at::empty({R, S, 1}, o), at::empty({R, S, 1}, o), at::empty({R, S, 1}, o),
                             at::empty({R, S, 1}, o), at::empty({R}, o), at::empty({R}, o), at::empty({R, 3}, o), at::empty({R}, o)};
    snerf_composite_out co{mptr(r[0]), mptr(r[1]), mptr(r[2]), mptr(r[3]), mptr(r[4]), mptr(r[5]), mptr(r[6]), mptr(r[7]), mptr(r[8]), mptr(r[9])};
    ck(snerf_composite_rays(R, (int)S, fptr(top), fptr(bot), fptr(tvals), fptr(rho), fptr(col), fptr(solar_vis), fptr(sky), (int)flags,
                            rho_prior.has_value() ? fptr(*rho_prior) : nullptr, (float)trust, &co, cur_stream(top)), "composite");
    return r;      // rgb, albedo, pv, pe, ps, delta, shadow, acc, surf_loc, surf_dist
}

std::vector<Tensor> composite_sweep(const Tensor& top, const Tensor& bot, const Tensor& tvals, const Tensor& rho, const Tensor& col_raw, const Tensor& adjust,
                                    const Tensor& solar_vis, const Tensor& sky, const Tensor& class_vecs, int64_t flags, bool classic) {
    check_shape(top, "top", -1, 3);
    const int64_t R = top.size(0);
    check_shape(bot, "bot", R, 3);
    check_dev_f32(tvals, "tvals");
    const int64_t S = tvals.numel();
    check_dev_f32(class_vecs, "class_vecs");
    TORCH_CHECK(class_vecs.dim() == 2, "class_vecs must be [T,C]");
    const int64_t T = class_vecs.size(0), C = class_vecs.size(1);
    check_dev_f32(rho, "rho"); check_dev_f32(col_raw, "col_raw"); check_dev_f32(adjust, "adjust"); check_dev_f32(solar_vis, "solar_vis"); check_dev_f32(sky, "sky");
    TORCH_CHECK(rho.numel() == R * S && solar_vis.numel() == R * S && col_raw.numel() == R * S * 3 && adjust.numel() == R * S * C * 3 && sky.numel() == 3,
                "per-sample tensors must hold R*S elements (col_raw x3, adjust xC x3), sky 3");
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    auto o = top.options();
    std::vector<Tensor> r = {at::empty({T, R, 3}, o), at::empty({T, R, 3}, o), at::empty({R, 3}, o), at::empty({R, 3}, o), at::empty({R}, o),
                             at::empty({classic ? T : 0, R, 3}, o)};
    snerf_sweep_out so{};
    so.d_season = mptr(r[0]); so.d_shaded = mptr(r[1]); so.d_base = mptr(r[2]); so.d_shadow_adjust = mptr(r[3]); so.d_raw_shadow = mptr(r[4]);
    so.d_classic = classic ? mptr(r[5]) : nullptr;
    ck(snerf_composite_sweep(R, (int)S, (int)C, (int)T, fptr(top), fptr(bot), fptr(tvals), nullptr, fptr(rho), fptr(col_raw), fptr(adjust), fptr(solar_vis),
                             fptr(sky), fptr(class_vecs), (int)flags, &so, cur_stream(top)), "composite_sweep");
    return r;      // season, shaded, base, shadow_adjust, raw_shadow, classic
}

// Sun walk (include/season_nerf_hip.h snerf_field_sun_walk_rays).  The model travels as an integer, as the trainer does below: the handle of a
// finalized model (Model.handle()), which the caller keeps alive.
std::vector<Tensor> sun_walk_fwd(int64_t model, const Tensor& top, const Tensor& bot, const Tensor& tvals, const Tensor& suns, const c10::optional<Tensor>& classes) {
    TORCH_CHECK(model != 0, "season_nerf::sun_walk_fwd: NULL model handle");
    const snerf_model* m = (const snerf_model*)model;
    const auto [R, S] = check_rays(top, bot, tvals);
    check_shape(suns, "suns", -1, 3);
    const int64_t M = suns.size(0), C = snerf_model_classes(m);
    TORCH_CHECK(M >= 1 && M <= 32, "suns must hold 1 to 32 directions per launch, got ", M);
    if (classes.has_value()) { check_dev_f32(*classes, "classes"); TORCH_CHECK(classes->numel() == C, "classes must hold ", C, " values, got ", classes->sizes()); }
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    auto o = top.options();
    std::vector<Tensor> r = {at::empty({R, S, 1}, o), at::empty({M, R, S, 1}, o), at::empty({R, S, 3}, o), at::empty({R, S, C, 3}, o), at::empty({R, S, 3}, o)};
    snerf_field_out fo{};
    fo.d_rho = mptr(r[0]); fo.d_solar_vis = mptr(r[1]); fo.d_col_raw = mptr(r[2]); fo.d_adjust = mptr(r[3]); fo.d_points = mptr(r[4]);
    ck(snerf_field_sun_walk_rays(m, R, (int)S, fptr(top), fptr(bot), fptr(tvals), (int)M, fptr(suns), classes.has_value() ? fptr(*classes) : nullptr, &fo,
                                 cur_stream(top)), "sun_walk_fwd");
    return r;      // rho, solar_vis, col_raw, adjust, points
}

// Ray surface (include/season_nerf_hip.h snerf_field_ray_surface): the four sums per ray a height map is formed from.  The model travels as an
// integer, as in sun_walk_fwd, so that the op has a fake kernel.
Tensor ray_surface(int64_t model, const Tensor& top, const Tensor& bot, const Tensor& tvals, int64_t flags) {
    TORCH_CHECK(model != 0, "season_nerf::ray_surface: NULL model handle");
    const auto [R, S] = check_rays(top, bot, tvals);
    TORCH_CHECK(flags >= 0 && (flags & ~(int64_t)6) == 0, "flags must be a combination of 2 (zero delta outside the cube) and 4 (no early-out), got ", flags);
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    Tensor out = at::empty({R, 4}, top.options());
    if (R == 0) return out;
    ck(snerf_field_ray_surface((const snerf_model*)model, R, (int)S, fptr(top), fptr(bot), fptr(tvals), (int)flags, mptr(out), cur_stream(top)), "ray_surface");
    return out;
}

// Shadow walk (include/season_nerf_hip.h snerf_field_shadow_walk): the eight sums per ray the reference's shadow scores are formed from.  The model
// travels as an integer, as in ray_surface.
Tensor shadow_walk(int64_t model, const Tensor& top, const Tensor& bot, const Tensor& sun, const Tensor& tvals, int64_t flags) {
    TORCH_CHECK(model != 0, "season_nerf::shadow_walk: NULL model handle");
    const auto [R, S] = check_rays(top, bot, tvals);
    check_shape(sun, "sun", R, 3);
    TORCH_CHECK(flags == 0 || flags == 2, "flags must be 0 or 2 (zero delta outside the cube), got ", flags);
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    Tensor out = at::empty({R, 8}, top.options());
    if (R == 0) return out;
    ck(snerf_field_shadow_walk((const snerf_model*)model, R, (int)S, fptr(top), fptr(bot), fptr(sun), fptr(tvals), (int)flags, mptr(out),
                               cur_stream(top)), "shadow_walk");
    return out;
}

// Solar audit (include/season_nerf_hip.h snerf_field_solar_audit): the eight sums per primary ray the reference's solar audit is formed from, and Exact_Solar
// per sample if asked for ([0] otherwise).  The sun travels as three float64 values; the model as an integer, as in ray_surface.
std::tuple<Tensor, Tensor> solar_audit(int64_t model, const Tensor& top, const Tensor& bot, const Tensor& tvals, c10::ArrayRef<double> sun, const Tensor& est_vis,
                                       const Tensor& ps, int64_t flags, bool want_exact) {
    TORCH_CHECK(model != 0, "season_nerf::solar_audit: NULL model handle");
    const auto [R, S] = check_rays(top, bot, tvals);
    TORCH_CHECK(sun.size() == 3, "sun must hold 3 values, got ", sun.size());
    TORCH_CHECK(std::isfinite(sun[0]) && std::isfinite(sun[1]) && std::isfinite(sun[2]) && sun[2] > 0.0 && (float)sun[2] > 0.f,
                "sun must be finite with sun_z > 0, got (", sun[0], ", ", sun[1], ", ", sun[2], ")");
    check_dev_f32(est_vis, "est_vis");
    check_dev_f32(ps, "ps");
    TORCH_CHECK(est_vis.numel() == R * S, "est_vis must hold R*S = ", R * S, " values, got ", est_vis.sizes());
    TORCH_CHECK(ps.numel() == R * S, "ps must hold R*S = ", R * S, " values, got ", ps.sizes());
    TORCH_CHECK(flags >= 0 && (flags & ~(int64_t)6) == 0, "flags must be a combination of 2 (zero delta outside the cube) and 4 (no early-out), got ", flags);
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    Tensor out = at::empty({R, 8}, top.options());
    Tensor exact = at::empty({want_exact ? R : 0, want_exact ? S : 0}, top.options());
    if (R == 0) return {out, exact};
    const double s3[3] = {sun[0], sun[1], sun[2]};
    ck(snerf_field_solar_audit((const snerf_model*)model, R, (int)S, fptr(top), fptr(bot), fptr(tvals), s3, fptr(est_vis), fptr(ps), (int)flags, mptr(out),
                               want_exact ? mptr(exact) : nullptr, cur_stream(top)), "solar_audit");
    return {out, exact};
}

// Frame walk (include/season_nerf_hip.h snerf_field_frame_walk): sixteen sums per ray of a film frame, up to four seasons from one field pass.  The model
// travels as an integer, as in ray_surface.
Tensor frame_walk(int64_t model, const Tensor& top, const Tensor& bot, const Tensor& tvals, double delta, const Tensor& sun, const Tensor& sky,
                  const Tensor& class_vecs, int64_t flags) {
    TORCH_CHECK(model != 0, "season_nerf::frame_walk: NULL model handle");
    const auto [R, S] = check_rays(top, bot, tvals, 2);
    check_dev_f32(sun, "sun");
    check_dev_f32(sky, "sky");
    TORCH_CHECK(sun.dim() == 1 && sun.numel() == 3 && sky.dim() == 1 && sky.numel() == 3, "sun and sky must be [3]");
    check_shape(class_vecs, "class_vecs", -1, snerf_model_classes((const snerf_model*)model));
    TORCH_CHECK(class_vecs.size(0) >= 1 && class_vecs.size(0) <= SNERF_MAX_FRAME_TIMES, "class_vecs must be [T,C] with 1 <= T <= ", SNERF_MAX_FRAME_TIMES,
                ", got T = ", class_vecs.size(0));
    TORCH_CHECK(std::isfinite(delta) && delta > 0, "delta must be finite and positive, got ", delta);
    TORCH_CHECK((flags & ~(int64_t)6) == 0, "flags must be a combination of 2 (zero delta outside the cube) and 4 (no early-out), got ", flags);
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    Tensor out = at::empty({R, 16}, top.options());
    if (R == 0) return out;
    ck(snerf_field_frame_walk((const snerf_model*)model, R, (int)S, fptr(top), fptr(bot), fptr(tvals), (float)delta, fptr(sun), fptr(sky),
                              (int)class_vecs.size(0), fptr(class_vecs), (int)flags, mptr(out), cur_stream(top)), "frame_walk");
    return out;
}

std::vector<Tensor> composite_sun_walk(const Tensor& top, const Tensor& bot, const Tensor& tvals, const Tensor& rho, const Tensor& col_raw, const Tensor& adjust,
                                       const Tensor& solar_vis, const Tensor& sky, const Tensor& class_vecs, int64_t flags, const c10::optional<Tensor>& deltas) {
    check_shape(top, "top", -1, 3);
    const int64_t R = top.size(0);
    check_shape(bot, "bot", R, 3);
    check_dev_f32(tvals, "tvals");
    const int64_t S = tvals.numel();
    TORCH_CHECK(S >= 1, "tvals must be [S]");
    check_dev_f32(class_vecs, "class_vecs");
    TORCH_CHECK(class_vecs.dim() == 2, "class_vecs must be [T,C]");
    const int64_t T = class_vecs.size(0), C = class_vecs.size(1);
    check_shape(sky, "sky", -1, 3);
    const int64_t M = sky.size(0);
    check_dev_f32(rho, "rho"); check_dev_f32(col_raw, "col_raw"); check_dev_f32(adjust, "adjust"); check_dev_f32(solar_vis, "solar_vis");
    TORCH_CHECK(rho.numel() == R * S && solar_vis.numel() == M * R * S && col_raw.numel() == R * S * 3 && adjust.numel() == R * S * C * 3,
                "per-sample tensors must hold R*S elements (col_raw x3, adjust xC x3, solar_vis xM = the rows of sky)");
    if (deltas.has_value()) { check_dev_f32(*deltas, "deltas"); TORCH_CHECK(deltas->numel() == R * S, "deltas must hold R*S elements"); }
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    auto o = top.options();
    std::vector<Tensor> r = {at::empty({M, T, R, 3}, o), at::empty({T, R, 3}, o), at::empty({R, 3}, o), at::empty({M, R}, o), at::empty({M, R, 3}, o)};
    snerf_sun_walk_out so{mptr(r[0]), mptr(r[1]), mptr(r[2]), mptr(r[3]), mptr(r[4])};
    ck(snerf_composite_sun_walk(R, (int)S, (int)C, (int)T, (int)M, fptr(top), fptr(bot), fptr(tvals), deltas.has_value() ? fptr(*deltas) : nullptr, fptr(rho),
                                fptr(col_raw), fptr(adjust), fptr(solar_vis), fptr(sky), fptr(class_vecs), (int)flags, &so, cur_stream(top)), "composite_sun_walk");
    return r;      // shaded, season, base, raw_shadow, shadow_adjust
}

void fused_adam_(Tensor param, const Tensor& grad, Tensor m, Tensor v, double lr, double beta1, double beta2, double eps, int64_t step) {
    check_dev_f32(param, "param"); check_dev_f32(grad, "grad"); check_dev_f32(m, "m"); check_dev_f32(v, "v");
    TORCH_CHECK(grad.numel() == param.numel() && m.numel() == param.numel() && v.numel() == param.numel(), "param, grad, m and v must have the same size");
    c10::hip::HIPGuardMasqueradingAsCUDA g(param.device());
    ck(snerf_adam_step(mptr(param), fptr(grad), mptr(m), mptr(v), param.numel(), (float)lr, (float)beta1, (float)beta2, (float)eps, (int)step,
                       cur_stream(param)), "fused_adam_");
}

// ---- training engine ---------------------------------------------------------------------------------------------------
// The trainer travels through the op schemas as an integer: never dereference it before the library has confirmed it is a live trainer;
// n_classes >= 0: must be the trainer's class count (the passes write [.., C] arrays sized by the caller).
snerf_trainer* trainer_of(int64_t h, int64_t n_classes = -1) {
    TORCH_CHECK(h != 0, "season_nerf::train_*: NULL trainer handle");
    const int c = snerf_trainer_classes((const snerf_trainer*)h);
    TORCH_CHECK(c > 0, "season_nerf::train_*: ", h, " is not the handle of a live training engine (destroyed, or never created)");
    TORCH_CHECK(n_classes < 0 || n_classes == c, "season_nerf::train_*: n_classes = ", n_classes, " but the engine was built for ", c, " classes");
    return (snerf_trainer*)h;
}
const float* optptr(const c10::optional<Tensor>& t, const char* name, int64_t numel) {
    if (!t.has_value()) return nullptr;
    check_dev_f32(*t, name);
    TORCH_CHECK(t->numel() == numel, name, " must hold ", numel, " elements, got ", t->sizes());
    return fptr(*t);
}

Tensor prior_density(const Tensor& pts, const Tensor& delta, const Tensor& height_map, const c10::optional<Tensor>& outside) {
    check_shape(pts, "pts", -1, 3);
    check_dev_f32(delta, "delta");
    const int64_t N = pts.size(0);
    TORCH_CHECK(delta.numel() == N, "delta must hold one value per point");
    TORCH_CHECK(height_map.is_cuda() && height_map.scalar_type() == at::kDouble && height_map.dim() == 2 && height_map.is_contiguous(),
                "height_map must be a contiguous float64 [h, w] tensor on the GPU");
    c10::hip::HIPGuardMasqueradingAsCUDA g(pts.device());
    Tensor out = at::empty({N, 1}, pts.options());
    ck(snerf_prior_density(N, fptr(pts), fptr(delta), height_map.data_ptr<double>(), (int)height_map.size(0), (int)height_map.size(1),
                           optptr(outside, "outside", N), mptr(out), cur_stream(pts)), "prior_density");
    return out;
}

std::vector<Tensor> train_fwd_image(int64_t trainer, const Tensor& top, const Tensor& bot, const Tensor& tvals, const Tensor& sun, const Tensor& time,
                                    bool train_bn, bool classic, int64_t n_classes, const c10::optional<Tensor>& height_map, double trust,
                                    const c10::optional<Tensor>& trust_dev, at::TensorList /*params*/) {
    snerf_trainer* t = trainer_of(trainer, n_classes);
    const auto [R, S] = check_rays(top, bot, tvals);
    check_shape(sun, "sun", R, 3); check_shape(time, "time", R, 4);
    TORCH_CHECK(n_classes >= 1 && n_classes <= 5, "n_classes must be in [1, 5]");
    const int64_t C = n_classes;
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    auto o = top.options();
    auto e = [&](std::initializer_list<int64_t> sz) { return at::empty(sz, o); };
    Tensor rgb = e({R, 3}), albedo = e({R, 3}), sky = e({R, 3}), pe = e({R, S, 1}), pv = e({R, S, 1}), ps = e({R, S, 1}), delta = e({R, S, 1}),
           cls = e({R, C}), rho = e({R, S, 1}), sv = e({R, S, 1}), col = e({R, S, 3}), pts = e({R, S, 3}), adjc = e({R, S, 3});
    snerf_composite_out co{};
    co.d_rgb = mptr(rgb); co.d_albedo = mptr(albedo); co.d_pv = mptr(pv); co.d_pe = mptr(pe); co.d_ps = mptr(ps); co.d_delta = mptr(delta);
    snerf_field_out fo{};
    fo.d_rho = mptr(rho); fo.d_solar_vis = mptr(sv); fo.d_col = mptr(col); fo.d_points = mptr(pts); fo.d_adjust_col = mptr(adjc);
    void* st = cur_stream(top);
    ck(snerf_trainer_forward_image(t, R, (int)S, fptr(top), fptr(bot), fptr(tvals), fptr(sun), fptr(time), train_bn ? 1 : 0, classic ? 1 : 0, &co,
                                   mptr(sky), mptr(cls), &fo, st), "train_fwd_image");
    Tensor rgb_m = e({0}), alb_m = e({0});
    std::vector<Tensor> extra;
    if (height_map.has_value()) {      // DSM-prior phase (Eval_Tools_2.py:218-248): supervised density, merged density, their composites
        Tensor rs = prior_density(pts.reshape({-1, 3}), delta.reshape({-1}), *height_map, c10::nullopt).reshape({R, S, 1});
        // trust_dev (one float on the device) replaces `trust` where a captured step needs a factor that changes between replays
        const float* td = trust_dev.has_value() ? optptr(trust_dev, "trust_dev", 1) : nullptr;
        auto comp = [&](const Tensor& rho_t, const float* prior, float tr, int flags, Tensor* c_rgb, Tensor* c_alb, Tensor* c_pv, Tensor* c_pe, Tensor* c_ps) {
            snerf_composite_out c{};
            if (c_rgb) c.d_rgb = mptr(*c_rgb);
            if (c_alb) c.d_albedo = mptr(*c_alb);
            if (c_pv) c.d_pv = mptr(*c_pv);
            if (c_pe) c.d_pe = mptr(*c_pe);
            if (c_ps) c.d_ps = mptr(*c_ps);
            if (prior && td)
                ck(snerf_composite_rays_dt(R, (int)S, fptr(top), fptr(bot), fptr(tvals), fptr(rho_t), fptr(col), fptr(sv), fptr(sky), flags, prior, td, &c, st),
                   "train_fwd_image (prior composites)");
            else
                ck(snerf_composite_rays(R, (int)S, fptr(top), fptr(bot), fptr(tvals), fptr(rho_t), fptr(col), fptr(sv), fptr(sky), flags, prior, tr, &c, st),
                   "train_fwd_image (prior composites)");
        };
        Tensor pv_s = e({R, S, 1}), pe_s = e({R, S, 1}), ps_s = e({R, S, 1}), pv_m = e({R, S, 1}), pe_m = e({R, S, 1}), ps_m = e({R, S, 1});
        comp(rs, nullptr, 1.f, 0, nullptr, nullptr, &pv_s, &pe_s, &ps_s);
        rgb_m = e({R, 3}); alb_m = e({R, 3});
        comp(rho, fptr(rs), (float)trust, classic ? 1 : 0, &rgb_m, &alb_m, nullptr, nullptr, nullptr);
        Tensor rho_m = td ? rho * (*trust_dev) + rs * (1.0 - *trust_dev) : rho * trust + rs * (1.0 - trust);
        comp(rho_m, nullptr, 1.f, 0, nullptr, nullptr, &pv_m, &pe_m, &ps_m);
        extra = {rs, pv_s, pe_s, ps_s, pv_m, pe_m, ps_m, rho_m};
    }
    std::vector<Tensor> r = {rgb, albedo, sky, pe, rgb_m, alb_m, pv, ps, delta, cls, rho, sv, col, pts, adjc};
    r.insert(r.end(), extra.begin(), extra.end());
    return r;
}

void train_bwd_image(int64_t trainer, Tensor grads, const c10::optional<Tensor>& g_rgb, const c10::optional<Tensor>& g_albedo, const c10::optional<Tensor>& g_sky,
                     const c10::optional<Tensor>& g_pe, const c10::optional<Tensor>& rho_prior, double trust, const c10::optional<Tensor>& g_rgb_m,
                     const c10::optional<Tensor>& g_alb_m, int64_t n_rays, int64_t n_samples, const c10::optional<Tensor>& trust_dev) {
    snerf_trainer* t = trainer_of(trainer);
    check_dev_f32(grads, "grads");
    const int64_t R = n_rays, N = n_rays * n_samples;
    c10::hip::HIPGuardMasqueradingAsCUDA g(grads.device());
    const float* prior = optptr(rho_prior, "rho_prior", N);
    const float* gm = prior ? optptr(g_rgb_m, "g_rgb_merged", R * 3) : nullptr;
    const float* ga = prior ? optptr(g_alb_m, "g_albedo_merged", R * 3) : nullptr;
    if (prior && trust_dev.has_value())
        ck(snerf_trainer_backward_image_dt(t, optptr(g_rgb, "g_rgb", R * 3), optptr(g_albedo, "g_albedo", R * 3), optptr(g_sky, "g_sky", R * 3),
                                           optptr(g_pe, "g_pe", N), prior, optptr(trust_dev, "trust_dev", 1), gm, ga, cur_stream(grads)), "train_bwd_image");
    else
        ck(snerf_trainer_backward_image(t, optptr(g_rgb, "g_rgb", R * 3), optptr(g_albedo, "g_albedo", R * 3), optptr(g_sky, "g_sky", R * 3), optptr(g_pe, "g_pe", N),
                                        prior, (float)trust, gm, ga, cur_stream(grads)), "train_bwd_image");
}

std::vector<Tensor> train_fwd_points(int64_t trainer, const Tensor& x, const Tensor& sun, const Tensor& time, bool train_bn, int64_t n_classes,
                                     at::TensorList /*params*/) {
    snerf_trainer* t = trainer_of(trainer, n_classes);
    check_shape(x, "x", -1, 3);
    const int64_t N = x.size(0), C = n_classes;
    check_shape(sun, "sun", N, 3); check_shape(time, "time", N, 4);
    TORCH_CHECK(n_classes >= 1 && n_classes <= 5, "n_classes must be in [1, 5]");
    c10::hip::HIPGuardMasqueradingAsCUDA g(x.device());
    auto o = x.options();
    Tensor rho = at::empty({N, 1}, o), col = at::empty({N, 3}, o), sv = at::empty({N, 1}, o), sky = at::empty({N, 3}, o), cls = at::empty({N, C}, o),
           adjc = at::empty({N, 3}, o), col_raw = at::empty({N, 3}, o), adj = at::empty({N, C, 3}, o), rgb = at::empty({N, 3}, o), tv = at::zeros({1}, o);
    snerf_composite_out co{};
    co.d_rgb = mptr(rgb);
    snerf_field_out fo{};
    fo.d_rho = mptr(rho); fo.d_solar_vis = mptr(sv); fo.d_col = mptr(col); fo.d_adjust_col = mptr(adjc); fo.d_col_raw = mptr(col_raw); fo.d_adjust = mptr(adj);
    // N rays of one sample at t = 0: point = Top (per-point sun / time, as the reference's evaluator passes them, Eval_Tools_2.py:174-176)
    ck(snerf_trainer_forward_image(t, N, 1, fptr(x), fptr(x), fptr(tv), fptr(sun), fptr(time), train_bn ? 1 : 0, 0, &co, mptr(sky), mptr(cls), &fo,
                                   cur_stream(x)), "train_fwd_points");
    return {rho, col, sv, sky, cls, adjc, col_raw, adj};
}

void train_bwd_points(int64_t trainer, Tensor grads, const c10::optional<Tensor>& g_rho, const c10::optional<Tensor>& g_col, const c10::optional<Tensor>& g_sv,
                      const c10::optional<Tensor>& g_sky, const c10::optional<Tensor>& g_cls, int64_t n_points, int64_t n_classes) {
    snerf_trainer* t = trainer_of(trainer, n_classes);
    check_dev_f32(grads, "grads");
    const int64_t N = n_points;
    c10::hip::HIPGuardMasqueradingAsCUDA g(grads.device());
    ck(snerf_trainer_backward_points(t, optptr(g_rho, "g_rho", N), optptr(g_col, "g_col", N * 3), optptr(g_sv, "g_solar_vis", N), optptr(g_sky, "g_sky", N * 3),
                                     optptr(g_cls, "g_classes", N * n_classes), cur_stream(grads)), "train_bwd_points");
}

std::vector<Tensor> train_fwd_solar(int64_t trainer, const Tensor& top, const Tensor& bot, const Tensor& tvals, const Tensor& sun, bool train_bn,
                                    at::TensorList /*params*/) {
    snerf_trainer* t = trainer_of(trainer);
    const auto [R, S] = check_rays(top, bot, tvals);
    check_shape(sun, "sun", R, 3);
    c10::hip::HIPGuardMasqueradingAsCUDA g(top.device());
    auto o = top.options();
    Tensor sv = at::empty({R, S, 1}, o), pv = at::empty({R, S, 1}, o), pe = at::empty({R, S, 1}, o), sky_raw = at::empty({R, 3}, o), rho = at::empty({R, S, 1}, o),
           pts = at::empty({R, S, 3}, o), dl = at::empty({R, S, 1}, o);
    ck(snerf_trainer_forward_solar(t, R, (int)S, fptr(top), fptr(bot), fptr(tvals), fptr(sun), train_bn ? 1 : 0, mptr(sv), mptr(pv), mptr(pe), mptr(sky_raw),
                                   mptr(rho), mptr(pts), mptr(dl), cur_stream(top)), "train_fwd_solar");
    return {sv, pv, pe, sky_raw, rho, pts, dl};
}

void train_bwd_solar(int64_t trainer, Tensor grads, const Tensor& g_sv) {
    snerf_trainer* t = trainer_of(trainer);
    check_dev_f32(grads, "grads");
    check_dev_f32(g_sv, "g_solar_vis");
    int64_t rs = 0;
    int ns = 0;
    ck(snerf_trainer_bound_sizes(t, nullptr, &rs, &ns), "train_bwd_solar");
    TORCH_CHECK(g_sv.numel() == rs * ns, "g_solar_vis must hold ", rs * ns, " elements (the sun rays x samples of the forward), got ", g_sv.sizes());
    c10::hip::HIPGuardMasqueradingAsCUDA g(grads.device());
    ck(snerf_trainer_backward_solar(t, fptr(g_sv), cur_stream(grads)), "train_bwd_solar");
}

// ---- the engine's optimiser step and gradient reset as ops (dispatcher- and profiler-visible; `params` / `grads` are the flat arenas the trainer is bound to)
void trainer_adam_step_(int64_t trainer, Tensor params, const Tensor& grads, double lr, double beta1, double beta2, double eps, int64_t step) {
    snerf_trainer* t = trainer_of(trainer);
    check_dev_f32(params, "params"); check_dev_f32(grads, "grads");
    TORCH_CHECK(grads.numel() == params.numel() && params.numel() == snerf_trainer_param_floats(t), "params / grads must be the trainer's flat arenas (",
                snerf_trainer_param_floats(t), " floats)");
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    ck(snerf_trainer_adam_step(t, (float)lr, (float)beta1, (float)beta2, (float)eps, (int)step, cur_stream(params)), "trainer_adam_step_");
}
void trainer_adam_step_dev_(int64_t trainer, Tensor params, const Tensor& grads, const Tensor& hyper) {
    snerf_trainer* t = trainer_of(trainer);
    check_dev_f32(params, "params"); check_dev_f32(grads, "grads"); check_dev_f32(hyper, "hyper");
    TORCH_CHECK(hyper.numel() == 6, "hyper must hold [lr, beta1, beta2, eps, 1 - beta1^t, 1 - beta2^t]");
    TORCH_CHECK(grads.numel() == params.numel() && params.numel() == snerf_trainer_param_floats(t), "params / grads must be the trainer's flat arenas");
    c10::hip::HIPGuardMasqueradingAsCUDA g(params.device());
    ck(snerf_trainer_adam_step_dev(t, fptr(hyper), cur_stream(params)), "trainer_adam_step_dev_");
}
void trainer_zero_grad_(int64_t trainer, Tensor grads) {
    snerf_trainer* t = trainer_of(trainer);
    check_dev_f32(grads, "grads");
    TORCH_CHECK(grads.numel() == snerf_trainer_param_floats(t), "grads must be the trainer's flat gradient arena");
    c10::hip::HIPGuardMasqueradingAsCUDA g(grads.device());
    ck(snerf_trainer_zero_grad(t, cur_stream(grads)), "trainer_zero_grad_");
}

// the block-sum scratch of loss_terms_all: one per (device, stream), created at first use; launches of one stream are serialised, and the scratch needs no
// initial state (snerf_loss_all_forward).  (One scratch per DEVICE would let two streams of a device - a captured step on its side stream next to an eager
// validation step, two networks trained side by side - mix their sums.)
static Tensor loss_all_scratch(const Tensor& like) {
    static std::mutex mu;
    static auto* per_stream = new std::map<std::pair<int, void*>, Tensor>();
    std::lock_guard<std::mutex> lock(mu);
    Tensor& s = (*per_stream)[{like.get_device(), cur_stream(like)}];
    if (!s.defined()) s = at::empty({(int64_t)snerf_loss_all_scratch_bytes()}, like.options().dtype(at::kByte));
    return s;
}
// Create the scratch of the CURRENT stream now: a captured step calls this on its capture stream BEFORE the capture begins, so that the capture does not
// allocate it from the graph's private pool.
void loss_scratch_prepare(const Tensor& like) {
    check_dev_f32(like, "like");
    c10::hip::HIPGuardMasqueradingAsCUDA g(like.device());
    (void)loss_all_scratch(like);
}

// ---- scalar loss terms of a training step (get_loss, Eval_Tools_2.py:340-450; snerf_loss_all_*): values, their weight vector, what the backward needs ----
struct LossAllIn {
    const Tensor &rgb, &gt, &albedo, &sky, &sv, &pv, &pe_sun;
    const c10::optional<Tensor> &rgb_merged, &pe, &pe_sup, &alpha_c, &scale_c, &alpha_a, &scale_a, &logz_v, &logz_s, &alb_min_global;
};
static snerf_loss_in loss_all_in(const LossAllIn& t, int64_t world, int64_t flags, double w_solar, double w_color, double w_alpha, bool with_table = true) {
    check_shape(t.rgb, "rgb", -1, 3);
    const int64_t R = t.rgb.size(0);
    check_shape(t.gt, "gt", R, 3); check_shape(t.albedo, "albedo", R, 3); check_shape(t.sky, "sky", R, 3);
    check_dev_f32(t.sv, "solar_vis"); check_dev_f32(t.pv, "pv_exact"); check_dev_f32(t.pe_sun, "pe_solar");
    TORCH_CHECK(t.sv.dim() >= 2 && t.pv.numel() == t.sv.numel() && t.pe_sun.numel() == t.sv.numel(), "solar_vis, pv_exact and pe_solar must be [Rs, S(, 1)] tensors of one size");
    const int64_t Rs = t.sv.size(0), S = t.sv.numel() / Rs;
    TORCH_CHECK(world >= 1, "world must be >= 1");
    TORCH_CHECK(flags >= 0 && flags <= 7, "flags must combine the adaptive colour loss (1), the prior phase (2) and a detached sky term (4)");
    const bool ada = flags & SNERF_LOSS_ADAPTIVE, prior = flags & SNERF_LOSS_PRIOR;
    TORCH_CHECK(!ada || (t.alpha_c.has_value() && t.scale_c.has_value() && (!with_table || (t.logz_v.has_value() && t.logz_s.has_value()))), "the adaptive colour loss needs alpha_color, scale_color, logz_value, logz_slope");
    TORCH_CHECK(!prior || (t.pe.has_value() && t.pe_sup.has_value()), "the prior phase needs pe and pe_supervised");
    TORCH_CHECK(!(ada && prior) || (t.alpha_a.has_value() && t.scale_a.has_value()), "the adaptive loss in the prior phase needs alpha_alpha and scale_alpha");
    snerf_loss_in in{};
    in.n_rays = R; in.n_solar_rays = Rs; in.n_samples = (int)S; in.flags = (int)flags;
    in.d_rgb = fptr(t.rgb); in.d_rgb_merged = optptr(t.rgb_merged, "rgb_merged", R * 3); in.d_gt = fptr(t.gt); in.d_albedo = fptr(t.albedo); in.d_sky = fptr(t.sky);
    in.d_solar_vis = fptr(t.sv); in.d_pv_exact = fptr(t.pv); in.d_pe_solar = fptr(t.pe_sun);
    if (prior) { in.d_pe = optptr(t.pe, "pe", R * S); in.d_pe_supervised = optptr(t.pe_sup, "pe_supervised", R * S); }
    if (ada) {
        in.d_alpha_color = optptr(t.alpha_c, "alpha_color", 3); in.d_scale_color = optptr(t.scale_c, "scale_color", 3);
        if (with_table) {
            for (const auto* tb : {&*t.logz_v, &*t.logz_s})
                TORCH_CHECK(tb->is_cuda() && tb->scalar_type() == at::kDouble && tb->is_contiguous() && tb->numel() == 513, "logz_value / logz_slope must be contiguous float64 GPU tensors of 513 elements");
            in.d_logz_value = t.logz_v->data_ptr<double>(); in.d_logz_slope = t.logz_s->data_ptr<double>();
        }
        if (prior) { in.d_alpha_alpha = optptr(t.alpha_a, "alpha_alpha", 1); in.d_scale_alpha = optptr(t.scale_a, "scale_alpha", 1); }
    }
    in.d_albedo_min_global = optptr(t.alb_min_global, "albedo_min_global", 3);
    in.world = (int)world; in.w_solar = (float)w_solar; in.w_color = (float)w_color; in.w_alpha = (float)w_alpha;
    return in;
}
// loss_terms_all(...) -> (vals[n], weights[n], aux[14]);  loss_terms_all_bwd(g_vals, ..., aux) -> the ten gradients (an empty tensor where the configuration lacks the input)
std::tuple<Tensor, Tensor, Tensor> loss_terms_all(const Tensor& rgb, const c10::optional<Tensor>& rgb_merged, const Tensor& gt, const Tensor& albedo, const Tensor& sky,
                                                  const Tensor& sv, const Tensor& pv, const Tensor& pe_sun, const c10::optional<Tensor>& pe, const c10::optional<Tensor>& pe_sup,
                                                  const c10::optional<Tensor>& alpha_c, const c10::optional<Tensor>& scale_c, const c10::optional<Tensor>& alpha_a,
                                                  const c10::optional<Tensor>& scale_a, const c10::optional<Tensor>& logz_v, const c10::optional<Tensor>& logz_s,
                                                  const c10::optional<Tensor>& alb_min_global, int64_t world, int64_t flags, double w_solar, double w_color, double w_alpha) {
    const snerf_loss_in in = loss_all_in({rgb, gt, albedo, sky, sv, pv, pe_sun, rgb_merged, pe, pe_sup, alpha_c, scale_c, alpha_a, scale_a, logz_v, logz_s, alb_min_global},
                                         world, flags, w_solar, w_color, w_alpha);
    c10::hip::HIPGuardMasqueradingAsCUDA g(rgb.device());
    const int n = snerf_loss_all_term_count((int)flags);
    Tensor scratch = loss_all_scratch(rgb);
    Tensor vals = at::empty({n}, rgb.options()), wts = at::empty({n}, rgb.options()), aux = at::empty({14}, rgb.options());
    ck(snerf_loss_all_forward(&in, scratch.data_ptr(), mptr(vals), mptr(wts), mptr(aux), cur_stream(rgb)), "loss_terms_all");
    return {vals, wts, aux};
}
std::vector<Tensor> loss_terms_all_bwd(const Tensor& g_vals, const Tensor& rgb, const c10::optional<Tensor>& rgb_merged, const Tensor& gt, const Tensor& albedo, const Tensor& sky,
                                       const Tensor& sv, const Tensor& pv, const c10::optional<Tensor>& pe, const c10::optional<Tensor>& pe_sup,
                                       const c10::optional<Tensor>& alpha_c, const c10::optional<Tensor>& scale_c, const c10::optional<Tensor>& alpha_a,
                                       const c10::optional<Tensor>& scale_a, const Tensor& aux, int64_t flags) {
    const c10::optional<Tensor> none;
    // (the backward reads neither the sun rays' PE nor the table nor the global minimum: aux carries what the forward made of them; pv stands in for pe_solar)
    snerf_loss_in in = loss_all_in({rgb, gt, albedo, sky, sv, pv, pv, rgb_merged, pe, pe_sup, alpha_c, scale_c, alpha_a, scale_a, none, none, none}, 1, flags, 0, 0, 0, false);
    in.d_logz_value = in.d_logz_slope = (const double*)in.d_alpha_color;      // never read by the backward; non-NULL where the configuration is adaptive
    check_dev_f32(g_vals, "g_vals"); check_dev_f32(aux, "aux");
    TORCH_CHECK(g_vals.numel() == snerf_loss_all_term_count((int)flags) && aux.numel() == 14, "g_vals must hold one float per term, aux 14");
    c10::hip::HIPGuardMasqueradingAsCUDA g(rgb.device());
    auto like = [&](const c10::optional<Tensor>& t) { return t.has_value() ? at::empty_like(*t) : at::empty({0}, rgb.options()); };
    const bool ada = flags & SNERF_LOSS_ADAPTIVE, prior = flags & SNERF_LOSS_PRIOR;
    std::vector<Tensor> o = {at::empty_like(rgb), like(rgb_merged), at::empty_like(albedo), at::empty_like(sky), at::empty_like(sv), like(prior ? pe : none),
                             like(ada ? alpha_c : none), like(ada ? scale_c : none), like(ada && prior ? alpha_a : none), like(ada && prior ? scale_a : none)};
    auto p = [](Tensor& t) -> float* { return t.numel() ? t.data_ptr<float>() : nullptr; };
    const snerf_loss_grads G{p(o[0]), p(o[1]), p(o[2]), p(o[3]), p(o[4]), p(o[5]), p(o[6]), p(o[7]), p(o[8]), p(o[9])};
    ck(snerf_loss_all_backward(&in, fptr(aux), fptr(g_vals), &G, cur_stream(rgb)), "loss_terms_all_bwd");
    return o;
}

// ---- device ray loader: DataLoader(shuffle=True) + data_to_dict + SC_loader of mg_run_NeRF.py:74-84,122-133,229-264 as two kernel launches -----------
void loader_next(int64_t loader, const Tensor& table, const c10::optional<Tensor>& img_pt, const c10::optional<Tensor>& top, const c10::optional<Tensor>& bot,
                 const c10::optional<Tensor>& view, const c10::optional<Tensor>& sun, const c10::optional<Tensor>& time, const c10::optional<Tensor>& weight,
                 const c10::optional<Tensor>& gt, const c10::optional<Tensor>& index, const c10::optional<Tensor>& sc_top, const c10::optional<Tensor>& sc_bot) {
    snerf_loader* l = (snerf_loader*)loader;
    TORCH_CHECK(l, "loader_next: NULL loader handle");
    check_shape(table, "table", -1, 22);
    const int64_t B = snerf_loader_batch(l);
    auto out = [&](const c10::optional<Tensor>& t, const char* name, int64_t w) -> float* {
        if (!t.has_value()) return nullptr;
        check_dev_f32(*t, name);
        TORCH_CHECK(t->device() == table.device() && t->dim() == 2 && t->size(0) >= B && t->size(1) == w, name, " must be [>= ", B, ", ", w, "] on the table's device, got ", t->sizes());
        return t->data_ptr<float>();
    };
    snerf_loader_out o{};
    o.d_img_pt = out(img_pt, "img_pt", 2); o.d_top = out(top, "top", 3); o.d_bot = out(bot, "bot", 3); o.d_view_angle = out(view, "view_angle", 3);
    o.d_sun_angle = out(sun, "sun_angle", 3); o.d_time_encoded = out(time, "time_encoded", 4); o.d_sample_weight = out(weight, "sample_weight", 1);
    o.d_gt_color = out(gt, "gt_color", 3); o.d_sc_top = out(sc_top, "sc_top", 3); o.d_sc_bot = out(sc_bot, "sc_bot", 3);
    if (index.has_value()) {
        TORCH_CHECK(index->is_cuda() && index->device() == table.device() && index->scalar_type() == at::kLong && index->is_contiguous() && index->dim() == 1 && index->size(0) >= B,
                    "row_index must be a contiguous int64 [>= ", B, "] tensor on the table's device");
        o.d_row_index = index->data_ptr<int64_t>();
    }
    c10::hip::HIPGuardMasqueradingAsCUDA g(table.device());
    const int64_t rows = snerf_loader_next(l, &o, cur_stream(table));
    TORCH_CHECK(rows > 0, "season_nerf::loader_next failed (code ", rows, "): ", snerf_last_error());
}

// ---- per-step training inputs: sun rays, jitter and the schedule row drawn on the device (csrc/loader.hip), two kernel launches ------------------------
void step_inputs_draw(int64_t handle, const Tensor& table, const c10::optional<Tensor>& starts, const c10::optional<Tensor>& ends,
                      const c10::optional<Tensor>& vec, const c10::optional<Tensor>& times, const c10::optional<Tensor>& base, const c10::optional<Tensor>& tv_image,
                      const c10::optional<Tensor>& tv_solar, const c10::optional<Tensor>& hyper, const c10::optional<Tensor>& trust, const c10::optional<Tensor>& lr2) {
    snerf_step_inputs* h = (snerf_step_inputs*)handle;
    TORCH_CHECK(h, "step_inputs_draw: NULL handle");
    const int64_t n_rays = snerf_step_inputs_rays(h), n_samples = snerf_step_inputs_samples(h);
    check_shape(table, "table", snerf_step_inputs_table_rows(h), 8);      // the table the handle was created over (it reads that one)
    auto out = [&](const c10::optional<Tensor>& t, const char* name, int64_t numel) -> float* {
        if (!t.has_value()) return nullptr;
        check_dev_f32(*t, name);
        TORCH_CHECK(t->device() == table.device() && t->numel() == numel, name, " must hold ", numel, " floats on the table's device, got ", t->sizes());
        return t->data_ptr<float>();
    };
    snerf_step_inputs_out o{};
    o.d_starts = out(starts, "starts", n_rays * 3); o.d_ends = out(ends, "ends", n_rays * 3); o.d_vec = out(vec, "vec", n_rays * 3);
    o.d_times = out(times, "times", n_rays * 4); o.d_base = out(base, "base", n_samples); o.d_tv_image = out(tv_image, "tv_image", n_samples);
    o.d_tv_solar = out(tv_solar, "tv_solar", n_samples); o.d_hyper = out(hyper, "hyper", 6); o.d_trust = out(trust, "trust", 1); o.d_lr2 = out(lr2, "lr2", 1);
    c10::hip::HIPGuardMasqueradingAsCUDA g(table.device());
    ck(snerf_step_inputs_draw(h, &o, cur_stream(table)), "step_inputs_draw");
}

}  // namespace

TORCH_LIBRARY(season_nerf, m) {
    m.class_<Model>("Model")
        .def(torch::init<int64_t, int64_t, std::string>())
        .def("set_tensor", &Model::set_tensor)
        .def("finalize", &Model::finalize)
        .def("width", &Model::width)
        .def("classes", &Model::classes)
        .def("precision", &Model::precision)
        .def("resolve", &Model::resolve)
        .def("i8_estimate", &Model::i8_estimate)
        .def("handle", &Model::handle);
    m.def("model_from_handle(int handle) -> __torch__.torch.classes.season_nerf.Model", model_from_handle);
    m.def("group_fwd(__torch__.torch.classes.season_nerf.Model model, Tensor time, Tensor sun) -> (Tensor, Tensor, Tensor)");
    m.def("points_fwd(__torch__.torch.classes.season_nerf.Model model, Tensor x, Tensor? sun, Tensor? classes, int group_size, int variant) -> Tensor[]");
    m.def("ray_visibility(__torch__.torch.classes.season_nerf.Model model, Tensor top, Tensor bot, Tensor tvals, int flags) -> Tensor");
    m.def("render_fwd(__torch__.torch.classes.season_nerf.Model model, Tensor top, Tensor bot, Tensor sun, Tensor time, Tensor tvals, int flags, "
          "bool want_per_sample, bool want_unmixed=False) -> (Tensor, Tensor, Tensor, Tensor[])");
    m.def("composite(Tensor top, Tensor bot, Tensor tvals, Tensor rho, Tensor col, Tensor solar_vis, Tensor sky, int flags, Tensor? rho_prior, float trust) "
          "-> Tensor[]");
    m.def("composite_sweep(Tensor top, Tensor bot, Tensor tvals, Tensor rho, Tensor col_raw, Tensor adjust, Tensor solar_vis, Tensor sky, Tensor class_vecs, "
          "int flags, bool classic) -> Tensor[]");
    m.def("sun_walk_fwd(int model, Tensor top, Tensor bot, Tensor tvals, Tensor suns, Tensor? classes) -> Tensor[]");
    m.def("ray_surface(int model, Tensor top, Tensor bot, Tensor tvals, int flags) -> Tensor");
    m.def("shadow_walk(int model, Tensor top, Tensor bot, Tensor sun, Tensor tvals, int flags) -> Tensor");
    m.def("solar_audit(int model, Tensor top, Tensor bot, Tensor tvals, float[] sun, Tensor est_vis, Tensor ps, int flags, bool want_exact) -> (Tensor, Tensor)");
    m.def("frame_walk(int model, Tensor top, Tensor bot, Tensor tvals, float delta, Tensor sun, Tensor sky, Tensor class_vecs, int flags) -> Tensor");
    m.def("composite_sun_walk(Tensor top, Tensor bot, Tensor tvals, Tensor rho, Tensor col_raw, Tensor adjust, Tensor solar_vis, Tensor sky, Tensor class_vecs, "
          "int flags, Tensor? deltas=None) -> Tensor[]");
    m.def("fused_adam_(Tensor(a!) param, Tensor grad, Tensor(b!) m, Tensor(c!) v, float lr, float beta1, float beta2, float eps, int step) -> ()");
    m.def("prior_density(Tensor pts, Tensor delta, Tensor height_map, Tensor? outside) -> Tensor");
    m.def("trainer_adam_step_(int trainer, Tensor(a!) params, Tensor grads, float lr, float beta1, float beta2, float eps, int step) -> ()");
    m.def("trainer_adam_step_dev_(int trainer, Tensor(a!) params, Tensor grads, Tensor hyper) -> ()");
    m.def("trainer_zero_grad_(int trainer, Tensor(a!) grads) -> ()");
    m.def("loss_scratch_prepare(Tensor like) -> ()");
    m.def("loader_next(int loader, Tensor table, Tensor(a!)? img_pt, Tensor(b!)? top, Tensor(c!)? bot, Tensor(d!)? view_angle, Tensor(e!)? sun_angle, "
          "Tensor(f!)? time_encoded, Tensor(g!)? sample_weight, Tensor(h!)? gt_color, Tensor(i!)? row_index, Tensor(j!)? sc_top, Tensor(k!)? sc_bot) -> ()");
    m.def("step_inputs_draw(int handle, Tensor table, Tensor(a!)? starts, Tensor(b!)? ends, Tensor(c!)? vec, Tensor(d!)? times, Tensor? base, Tensor(e!)? tv_image, "
          "Tensor(f!)? tv_solar, Tensor(g!)? hyper, Tensor(h!)? trust, Tensor(i!)? lr2) -> ()");
    m.def("loss_terms_all(Tensor rgb, Tensor? rgb_merged, Tensor gt, Tensor albedo, Tensor sky, Tensor solar_vis, Tensor pv_exact, Tensor pe_solar, Tensor? pe, "
          "Tensor? pe_supervised, Tensor? alpha_color, Tensor? scale_color, Tensor? alpha_alpha, Tensor? scale_alpha, Tensor? logz_value, Tensor? logz_slope, "
          "Tensor? albedo_min_global, int world, int flags, float w_solar, float w_color, float w_alpha) -> (Tensor, Tensor, Tensor)");
    m.def("loss_terms_all_bwd(Tensor g_vals, Tensor rgb, Tensor? rgb_merged, Tensor gt, Tensor albedo, Tensor sky, Tensor solar_vis, Tensor pv_exact, Tensor? pe, "
          "Tensor? pe_supervised, Tensor? alpha_color, Tensor? scale_color, Tensor? alpha_alpha, Tensor? scale_alpha, Tensor aux, int flags) -> Tensor[]");
    m.def("train_fwd_image(int trainer, Tensor top, Tensor bot, Tensor tvals, Tensor sun, Tensor time, bool train_bn, bool classic, int n_classes, "
          "Tensor? height_map, float trust, Tensor? trust_dev, Tensor[] params) -> Tensor[]");
    m.def("train_bwd_image(int trainer, Tensor(a!) grads, Tensor? g_rgb, Tensor? g_albedo, Tensor? g_sky, Tensor? g_pe, Tensor? rho_prior, float trust, "
          "Tensor? g_rgb_merged, Tensor? g_albedo_merged, int n_rays, int n_samples, Tensor? trust_dev=None) -> ()");
    m.def("train_fwd_points(int trainer, Tensor x, Tensor sun, Tensor time, bool train_bn, int n_classes, Tensor[] params) -> Tensor[]");
    m.def("train_bwd_points(int trainer, Tensor(a!) grads, Tensor? g_rho, Tensor? g_col, Tensor? g_solar_vis, Tensor? g_sky, Tensor? g_classes, "
          "int n_points, int n_classes) -> ()");
    m.def("train_fwd_solar(int trainer, Tensor top, Tensor bot, Tensor tvals, Tensor sun, bool train_bn, Tensor[] params) -> Tensor[]");
    m.def("train_bwd_solar(int trainer, Tensor(a!) grads, Tensor g_solar_vis) -> ()");
}

TORCH_LIBRARY_IMPL(season_nerf, CUDA, m) {      // "CUDA" is the dispatch key of HIP tensors in PyTorch-ROCm
    m.impl("group_fwd", group_fwd);
    m.impl("points_fwd", points_fwd);
    m.impl("render_fwd", render_fwd);
    m.impl("ray_visibility", ray_visibility);
    m.impl("composite", composite);
    m.impl("composite_sweep", composite_sweep);
    m.impl("sun_walk_fwd", sun_walk_fwd);
    m.impl("composite_sun_walk", composite_sun_walk);
    m.impl("ray_surface", ray_surface);
    m.impl("shadow_walk", shadow_walk);
    m.impl("solar_audit", solar_audit);
    m.impl("frame_walk", frame_walk);
    m.impl("trainer_adam_step_", trainer_adam_step_);
    m.impl("trainer_adam_step_dev_", trainer_adam_step_dev_);
    m.impl("trainer_zero_grad_", trainer_zero_grad_);
    m.impl("loss_scratch_prepare", loss_scratch_prepare);
    m.impl("loader_next", loader_next);
    m.impl("step_inputs_draw", step_inputs_draw);
    m.impl("loss_terms_all", loss_terms_all);
    m.impl("loss_terms_all_bwd", loss_terms_all_bwd);
    m.impl("fused_adam_", fused_adam_);
    m.impl("prior_density", prior_density);
    m.impl("train_fwd_image", train_fwd_image);
    m.impl("train_bwd_image", train_bwd_image);
    m.impl("train_fwd_points", train_fwd_points);
    m.impl("train_bwd_points", train_bwd_points);
    m.impl("train_fwd_solar", train_fwd_solar);
    m.impl("train_bwd_solar", train_bwd_solar);
}
