"""The reference's solar audit (T_NeRF_Eval_Utils/mg_Advanced_Solar.py: `eval_solar_data`, `advanced_solar`, `_get_stats`, `_shadow_analyasis`): the sun
visibility the solar branch has learned (`Est_Solar_Vis`) against the one the density implies (`Exact_Solar`), sample by sample and at the surface
(sum_s vis PS > .3), over a grid of views and sun directions.

The reference renders every (view, sun) pair with `component_render_by_dir(..., include_exact_solar=True)` and counts on the host.  Here a view is walked
once: the sun walk gives rho and `Est_Solar_Vis` for all its sun directions from one field pass, `snerf_composite_rays` gives PS, and one launch of
`season_nerf::solar_audit` per sun direction (csrc/mlp_device.h RayAudit) forms the secondary rays in the kernel, walks them through the density-only network
and scores them there: eight numbers come back per primary ray (include/season_nerf_hip.h snerf_field_solar_audit), and no per-sample array unless asked for.
`eval_solar_data`, `advanced_solar`, `_get_stats` and `_shadow_analyasis` keep the reference's names and spelling."""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .evaluator import sample_parameters_on
from .render import (WALK_MAX_SUNS, WALK_SOLAR_VIS_BYTES, _exact_solar_visibility, _f32, _ray_grid, _walks, encode_time, world_angle_2_local_vec)

_KEYS = ("TP", "TN", "FP", "FN")


class SolarAudit:
    """What `solar_audit` returns: `sums` [M,R,8] float64 on the device, one row per sun direction and primary ray - `tp` = number of samples with
    Exact > .5 and Est > .5, `n_exact` = with Exact > .5, `n_est` = with Est > .5, `ps_exact` = sum Exact PS, `ps_est` = sum Est PS, `acc` = sum PS,
    `sq_err` = sum (Exact - Est)^2, `abs_err` = sum |Exact - Est| - and the reference's confusion counts formed from them."""

    _NAMES = ("tp", "n_exact", "n_est", "ps_exact", "ps_est", "acc", "sq_err", "abs_err")

    def __init__(self, sums, n_samples, exact=None):
        self.sums, self.n_samples, self._exact = sums, int(n_samples), exact

    def __getattr__(self, name):
        if name in SolarAudit._NAMES:
            return self.sums[..., SolarAudit._NAMES.index(name)]
        raise AttributeError(name)

    def __len__(self):
        return self.sums.shape[0]

    def exact(self, j):
        """`Exact_Solar` of sun direction j, [R,S] float32 on the device (only if the audit was asked for it: want_exact=True)."""
        if self._exact is None:
            raise ValueError("SolarAudit.exact: the audit was run without want_exact=True")
        return self._exact[j]

    def confusion(self, j=None):
        """The dict of `eval_solar_data` for sun direction j, or summed over every sun direction: integers, summed over the rays in int64.
        All_Solar_Vis: TP = tp, FN = n_exact - tp, FP = n_est - tp, TN = S - n_exact - n_est + tp per ray.  Surface_Solar_Vis: the rays by
        ps_exact > .3 and ps_est > .3."""
        s = (self.sums if j is None else self.sums[range(len(self))[j]]).reshape(-1, 8)
        tp, ne, nv = (s[:, k].round().to(torch.int64).sum() for k in range(3))
        total = s.shape[0] * self.n_samples
        g, e = s[:, 3] > .3, s[:, 4] > .3
        cnt = lambda m: int(m.to(torch.int64).sum().item())
        tp, ne, nv = int(tp.item()), int(ne.item()), int(nv.item())
        return {"All_Solar_Vis": {"TP": tp, "TN": total - ne - nv + tp, "FP": nv - tp, "FN": ne - tp},
                "Surface_Solar_Vis": {"TP": cnt(g & e), "TN": cnt(~g & ~e), "FP": cnt(~g & e), "FN": cnt(g & ~e)}}


def _sums_f64(exact, est, ps):
    """The eight sums per ray from per-sample arrays [R,S] in float64 (torch): what the kernel forms, for the paths without it."""
    ex, es = exact > .5, est > .5
    d = exact - est
    c = lambda m: m.sum(1).double()
    return torch.stack([c(ex & es), c(ex), c(es), (exact * ps).sum(1), (est * ps).sum(1), ps.sum(1), (d * d).sum(1), d.abs().sum(1)], 1)


def _composite_ps(R, S, top, bot, tv, rho, sv, st):
    """PS [R,S] of the primary rays: snerf_composite_rays with flags 2 (a sample outside the cube gets delta 0), as the renderers call it."""
    dev = top.device
    ps, z3 = torch.empty(R, S, 1, device=dev), torch.zeros(R, S, 3, device=dev)
    sky = torch.zeros(R, 3, device=dev)
    co = _lib.CompositeOut(d_ps=ps.data_ptr())
    _lib.check(_lib.lib().snerf_composite_rays(R, S, top.data_ptr(), bot.data_ptr(), tv.data_ptr(), rho.data_ptr(), z3.data_ptr(), sv.data_ptr(), sky.data_ptr(),
                                               2, None, 1.0, C.byref(co), st), "composite_rays")
    return ps.reshape(R, S)


def solar_audit(net, top, bot, sun_vecs, S, *, early_out=True, want_exact=False):
    """The solar audit of one view: primary rays top -> bot [R,3] (device) and M sun vectors `sun_vecs` (float64 [M,3], sun_z > 0) -> `SolarAudit`.
    S end-point-inclusive samples per ray, primary and secondary, as `component_render_by_dir(include_exact_solar=True)` lays them.

    On a fused bf16x3 model (widths 64 / 256 / 512) in eval mode: the sun walk in chunks of <= 32 sun directions (rho once, Est_Solar_Vis per sun - bit for
    bit the single-sun render's), one compositing launch for PS, one `season_nerf::solar_audit` launch per sun direction.  early_out=False walks every pass of
    every secondary ray; want_exact=True keeps `Exact_Solar` [M,R,S] for `.exact(j)`.
    Anything else (int8-resolved models, a width without a fused kernel, the one-term "bf16" mode, a module in training mode) gets the same numbers from
    `forward_Solar` on the sample points, `_exact_solar_visibility` and float64 sums: slower, and correct."""
    with torch.no_grad():
        suns64 = np.ascontiguousarray(np.asarray(sun_vecs, dtype=np.float64).reshape(-1, 3))
        M = suns64.shape[0]
        if M < 1:
            raise ValueError("solar_audit: at least one sun vector is needed")
        if not np.all(np.isfinite(suns64)) or not np.all(suns64[:, 2] > 0):
            raise ValueError("solar_audit: every sun vector must be finite with sun_z > 0")
        top, bot = net._prep(top, bot)
        if top.dim() != 2 or top.shape[1] != 3 or bot.shape != top.shape:
            raise ValueError(f"solar_audit: top {tuple(top.shape)} and bot {tuple(bot.shape)} must both be [R,3]")
        dev, R, S = top.device, top.shape[0], int(S)
        st = net._stream()
        tv = sample_parameters_on(dev, S, eval_mode=True, include_end_pt=True)
        sums = torch.zeros(M, R, 8, dtype=torch.float64, device=dev)
        exact = torch.empty(M, R, S, device=dev) if want_exact else None
        if R == 0:
            return SolarAudit(sums, S, exact)
        e = lambda *s: torch.empty(*s, device=dev)
        tim = _f32(encode_time(0.0).reshape(1, 4), dev)
        if _walks(net) and not net.training:
            from .network import _ops
            L, model = _lib.lib(), net.device_model()
            suns = _f32(suns64, dev)
            cls0 = net._groups(tim, suns[:1])[0][0].contiguous()
            rho, sv_all = e(R, S, 1), e(M, R, S, 1)
            for b0 in range(0, M, WALK_MAX_SUNS):
                b1 = min(M, b0 + WALK_MAX_SUNS)
                block = max(1, WALK_SOLAR_VIS_BYTES // (4 * S * (b1 - b0)))
                for r0 in range(0, R, block):
                    r1 = min(R, r0 + block)
                    whole = r0 == 0 and r1 == R
                    sv = sv_all[b0:b1] if whole else e(b1 - b0, r1 - r0, S, 1)
                    fo = _lib.FieldOut(d_solar_vis=sv.data_ptr()) if b0 else _lib.FieldOut(d_rho=rho[r0:r1].data_ptr(), d_solar_vis=sv.data_ptr())
                    _lib.check(L.snerf_field_sun_walk_rays(model, r1 - r0, S, top[r0:r1].data_ptr(), bot[r0:r1].data_ptr(), tv.data_ptr(), b1 - b0,
                                                           suns[b0:b1].data_ptr(), cls0.data_ptr(), C.byref(fo), st), "field_sun_walk_rays")
                    if not whole:
                        sv_all[b0:b1, r0:r1] = sv
            ps = _composite_ps(R, S, top, bot, tv, rho, sv_all[0], st)
            flags = 2 | (0 if early_out else 4)
            for j in range(M):
                out, ex = _ops().solar_audit(model, top, bot, tv, [float(x) for x in suns64[j]], sv_all[j].reshape(R, S), ps, flags, want_exact)
                sums[j] = out.double()
                if want_exact:
                    exact[j] = ex
            return SolarAudit(sums, S, exact)
        # fallback: the sample points formed as the kernels form them (two rounded products and a sum), density and learned visibility from forward_Solar
        pts = (top[:, None, :] * (1.0 - tv)[None, :, None] + bot[:, None, :] * tv[None, :, None]).reshape(-1, 3).contiguous()
        per = (1 << 20) if net.fused else min(1 << 16, max(64, int(12e9 / (128.0 * net.layer_width))))
        rho, ps = e(R * S), None
        for j in range(M):
            sun1 = _f32(suns64[j].reshape(1, 3), dev)
            vis = e(R * S)
            for i in range(0, R * S, per):
                p = pts[i:i + per]
                o = net.forward_Solar(p, sun1.expand(p.shape[0], 3), tim.expand(p.shape[0], 4))
                vis[i:i + per] = o[1].reshape(-1)
                if j == 0:
                    rho[i:i + per] = o[0].reshape(-1)
            if ps is None:
                ps = _composite_ps(R, S, top, bot, tv, rho.reshape(R, S, 1), vis.reshape(R, S, 1), st).double()
            ex = _exact_solar_visibility(net, pts, _f32(suns64[j], dev), S, zero_oob=True, sun64=suns64[j]).reshape(R, S)
            sums[j] = _sums_f64(ex.double(), vis.reshape(R, S).double(), ps)
            if want_exact:
                exact[j] = ex
        return SolarAudit(sums, S, exact)


def audit_by_dir(the_network, view_el_az, sun_el_azs, out_img_size, W2C, W2L_H, device, *, early_out=True, want_exact=False):
    """The audit of one view direction (el, az in degrees) under the sun directions `sun_el_azs` [(el, az), ...]: the ray grid of
    `component_render_by_dir` (mg_Img_Eval.py:96-115, out_img_size = (H, W, S)) and `world_angle_2_local_vec` for the suns -> `SolarAudit`, whose
    `.confusion(j)` is what `eval_solar_data(component_render_by_dir(..., sun_el_azs[j], ...))` counts."""
    Hh, Ww, S = out_img_size
    v = world_angle_2_local_vec(view_el_az[0], view_el_az[1], W2C, W2L_H)
    suns = np.stack([world_angle_2_local_vec(s[0], s[1], W2C, W2L_H) for s in sun_el_azs])
    with torch.no_grad():
        top, bot, _ = _ray_grid(0, Hh, Ww, v / v[2], device)
    return solar_audit(the_network, top, bot, suns, S, early_out=early_out, want_exact=want_exact)


def _confusion(gt, est, gt_surf, est_surf, count):
    c = lambda m: count(m)
    return {"All_Solar_Vis": {"TP": c(gt & est), "TN": c(~gt & ~est), "FP": c(~gt & est), "FN": c(gt & ~est)},
            "Surface_Solar_Vis": {"TP": c(gt_surf & est_surf), "TN": c(~gt_surf & ~est_surf), "FP": c(~gt_surf & est_surf), "FN": c(gt_surf & ~est_surf)}}


def eval_solar_data(rendered_dict):
    """mg_Advanced_Solar.py:11-37 on the dict of `component_render_by_dir(..., include_exact_solar=True)`: the confusion counts of Exact_Solar > .5 against
    Est_Solar_Vis > .5 over all samples, and of sum_s Exact PS > .3 against sum_s Est PS > .3 over the rays, PS = get_PV(Rho, Deltas) (1 - exp(-Rho Deltas)).
    An `ImgDict` that still has its device tensors is counted on the device (float64 there, nothing transferred but eight integers); a plain dict of numpy
    arrays is counted as the reference counts it, in float64 on the host."""
    d = getattr(rendered_dict, "dev", None)
    if d is not None and "Exact_Solar" in d and ("Deltas" in d or "Deltas_explicit" in d):
        with torch.no_grad():
            R, S = d["Rho"].shape[0], d["Rho"].shape[1]
            f = lambda k: d[k].reshape(R, S).double()
            ex, es = f("Exact_Solar"), f("Est_Solar_Vis")
            y = f("Rho") * f("Deltas" if "Deltas" in d else "Deltas_explicit")
            pv = torch.exp(-(torch.cumsum(y, 1) - y)) if S else y
            ps = pv * (1.0 - torch.exp(-y))
            return _confusion(ex > .5, es > .5, (ex * ps).sum(1) > .3, (es * ps).sum(1) > .3, lambda m: int(m.to(torch.int64).sum().item()))
    ex, es = np.asarray(rendered_dict["Exact_Solar"], dtype=np.float64), np.asarray(rendered_dict["Est_Solar_Vis"], dtype=np.float64)
    rho, dl = np.asarray(rendered_dict["Rho"], dtype=np.float64), np.asarray(rendered_dict["Deltas"], dtype=np.float64)
    y = rho * dl
    pv = np.exp(-np.cumsum(np.concatenate([np.zeros_like(y[:, :1]), y], 1), 1))[:, :-1]      # get_PV (Eval_Tools_2.py:13-16)
    ps = pv * (1 - np.exp(-y))
    return _confusion(ex > .5, es > .5, np.sum(ex * ps, 1) > .3, np.sum(es * ps, 1) > .3, lambda m: int(np.sum(m)))


def advanced_solar(the_network, W2C, W2L_H, device, out_img_size, sat_thetas=None, sat_el_phis=None, solar_thetas=None, solar_el_phis=None):
    """mg_Advanced_Solar.py:40-77 with the scene given directly (network, world centre, world-to-local matrix) instead of the reference's input dict: the
    confusion counts of every (view azimuth, view elevation, sun azimuth, sun elevation) of the grids - by default the reference's 4 x 3 x 6 x 4 - as its
    `Full_ans`.  One `audit_by_dir` per view: 12 field passes for the default grids where the reference renders 288 times.
    `Keys["Idx_2_sat_el"]` holds the view elevations (the reference stores the azimuths there a second time)."""
    sat_thetas = np.linspace(0, 360, 4, endpoint=False) if sat_thetas is None else np.asarray(sat_thetas, dtype=np.float64)
    sat_el_phis = np.linspace(60, 90, 3, endpoint=False) if sat_el_phis is None else np.asarray(sat_el_phis, dtype=np.float64)
    solar_thetas = np.linspace(0, 360, 6, endpoint=False) if solar_thetas is None else np.asarray(solar_thetas, dtype=np.float64)
    solar_el_phis = np.linspace(15, 90, 4, endpoint=False) if solar_el_phis is None else np.asarray(solar_el_phis, dtype=np.float64)
    shape = [sat_thetas.shape[0], sat_el_phis.shape[0], solar_thetas.shape[0], solar_el_phis.shape[0]]
    table = lambda: {"TP": -np.ones(shape, dtype=int), "TN": -np.ones(shape), "FP": -np.ones(shape), "FN": -np.ones(shape)}
    Full_ans = {"All_Solar_Vis": table(), "Surface_Solar_Vis": table(),
                "Keys": {"Idx_1_sat_azmuth": sat_thetas, "Idx_2_sat_el": sat_el_phis, "Idx_3_solar_azmuth": solar_thetas, "Idx_4_solar_el": solar_el_phis}}
    suns = [[solar_el_phis[ell], solar_thetas[k]] for k in range(shape[2]) for ell in range(shape[3])]
    for i in range(shape[0]):
        for j in range(shape[1]):
            audit = audit_by_dir(the_network, [sat_el_phis[j], sat_thetas[i]], suns, out_img_size, W2C, W2L_H, device)
            for n in range(len(suns)):
                ans = audit.confusion(n)
                for key1 in ans:
                    for key2 in ans[key1]:
                        Full_ans[key1][key2][i, j, n // shape[3], n % shape[3]] = ans[key1][key2]
    return Full_ans


_BASE_KEYS = ["Accuracy", "Accuracy_Balanced", "Shadow_Prevalence", "Solar_Precision", "Solar_Recall", "Shadow_Precision", "Shadow_Recall", "Solar_F1", "Shadow_F1"]


def _get_stats(TP, TN, FP, FN):
    """mg_Advanced_Solar.py:79-93 -> Acc, Acc_Balanced, Shadow_Prev, Prec_P, Recall_P, Prec_N, Recall_N, F1_P, F1_N; numpy's division: an empty class
    gives NaN, as in the reference (whose warnings are not repeated)."""
    TP, TN, FP, FN = (np.asarray(a, dtype=np.float64) for a in (TP, TN, FP, FN))
    with np.errstate(divide="ignore", invalid="ignore"):
        Acc = (TP + TN) / (TP + TN + FP + FN)
        Prec_P, Recall_P = TP / (TP + FP), TP / (TP + FN)
        Prec_N, Recall_N = TN / (TN + FN), TN / (TN + FP)
        Acc_Balanced = (Prec_P + Prec_N) / 2
        F1_P = 2 * Prec_P * Recall_P / (Prec_P + Recall_P)
        F1_N = 2 * Prec_N * Recall_N / (Prec_N + Recall_N)
        Shadow_Prev = (TN + FP) / (TP + TN + FP + FN)
    return Acc, Acc_Balanced, Shadow_Prev, Prec_P, Recall_P, Prec_N, Recall_N, F1_P, F1_N


def _shadow_analyasis(loaded_data):
    """mg_Advanced_Solar.py:95-144: for every region of {region: Full_ans} the nine statistics of `_get_stats` per grid cell and, under "Overall", of
    the counts summed over the grid - for All_Solar_Vis and for Surface_Solar_Vis.  Adds the keys in place and returns the dict, as the reference does."""
    for region in loaded_data:
        for family in ("All_Solar_Vis", "Surface_Solar_Vis"):
            t = loaded_data[region][family]
            TP, TN, FP, FN = (t[k] for k in _KEYS)
            for key, a in zip(_BASE_KEYS, _get_stats(TP, TN, FP, FN)):
                t[key] = a
            t["Overall"] = dict(zip(_BASE_KEYS, _get_stats(np.sum(TP), np.sum(TN), np.sum(FP), np.sum(FN))))
    return loaded_data
