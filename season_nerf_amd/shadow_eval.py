"""The reference's shadow test (T_NeRF_Eval_Utils/mg_Shadow_Eval.py, main_eval_region.py:77-84): along rays laid through ground points towards the sun,
the solar visibility the network has learned against the one its own density implies.

`shadow_walk` scores the rays inside the field kernel (`season_nerf::shadow_walk`, csrc/mlp_device.h RayShadow): eight sums per ray come back and no
per-sample array is ever formed; `ShadowWalk.scores` turns them into the eight numbers of `shadow_anaylysis`.  `eval_shadow_data`, `shadow_anaylysis` and
`Test_Shadow_Points` mirror the reference's call boundary with its spelling; `Test_Shadow_Points(full_return=False)` goes through `shadow_walk`.
"""
import numpy as np
import torch

from .evaluator import get_PV, sample_parameters_on
from .render import _f32, _ray_samples, _walks, world_angle_2_local_vec

SCORE_KEYS = ("Acc", "Prec_Sun", "Recall_Sun", "Prec_Shadow", "Recall_Shadow", "Loss", "Avg_Error", "Avg_Offset")


def _scores_from_sums(TP, n_exact, n_est, sq, ab, total, offset):
    """shadow_anaylysis' quotients (mg_Shadow_Eval.py:145-157) from float64 totals; an empty class gives NaN (or inf), as numpy's division does."""
    TP, n_exact, n_est, total = np.float64(TP), np.float64(n_exact), np.float64(n_est), np.float64(total)
    TN, FP, FN = total - n_exact - n_est + TP, n_est - TP, n_exact - TP
    with np.errstate(divide="ignore", invalid="ignore"):
        return {"Acc": (TP + TN) / (TP + TN + FP + FN), "Prec_Sun": TP / (TP + FP), "Recall_Sun": TP / (TP + FN), "Prec_Shadow": TN / (TN + FN),
                "Recall_Shadow": TN / (TN + FP), "Loss": np.float64(sq) / total, "Avg_Error": np.float64(ab) / total, "Avg_Offset": np.float64(offset)}


class ShadowWalk:
    """What `shadow_walk` returns: `sums` [..., 8] float32 on the device, one row per ray (include/season_nerf_hip.h snerf_field_shadow_walk) -
    `tp` = number of samples with PV > .5 and vis > .5, `n_exact` = with PV > .5, `n_est` = with vis > .5, `sq_err` = sum (PV - vis)^2,
    `abs_err` = sum |PV - vis|, `ps_vis` = sum PS vis, `acc` = sum PS, `carry` = the optical depth walked - and the reference's scores formed from them."""

    _NAMES = ("tp", "n_exact", "n_est", "sq_err", "abs_err", "ps_vis", "acc", "carry")

    def __init__(self, sums, n_samples):
        self.sums, self.n_samples = sums, int(n_samples)

    def __getattr__(self, name):
        if name in ShadowWalk._NAMES:
            return self.sums[..., ShadowWalk._NAMES.index(name)]
        raise AttributeError(name)

    def per_sun(self, M, G):
        """The same rows as [M, G]: sun direction by ground point, the order `Test_Shadow_Points` lays its rays in."""
        return ShadowWalk(self.sums.reshape(int(M), int(G), 8), self.n_samples)

    def scores(self, mask=None):
        """The dict of `shadow_anaylysis` (mg_Shadow_Eval.py:134-163) over all rays, or over those where the boolean `mask` is set, in float64:
        TN = S n - n_exact - n_est + TP, FP = n_est - TP, FN = n_exact - TP, Avg_Offset = mean |n_exact - n_est|."""
        s = self.sums.reshape(-1, 8).double()
        if mask is not None:
            s = s[torch.as_tensor(mask, device=s.device).reshape(-1).bool()]
        n = s.shape[0]
        tot = s[:, :5].sum(0).cpu().numpy()
        with np.errstate(invalid="ignore"):
            offset = (s[:, 1] - s[:, 2]).abs().mean().item() if n else np.float64("nan")
        return _scores_from_sums(tot[0], tot[1], tot[2], tot[3], tot[4], float(n) * self.n_samples, offset)


def _shadow_layerwise(net, tops, bots, suns, tv, S, zero_oob):
    """The eight numbers of `shadow_walk` for a chunk of rays from `forward_Solar` on the sample points and float64 sums: networks the shadow-walk
    kernels do not serve.  PV is the exclusive prefix formed as get_PV forms it (Eval_Tools_2.py:13-16)."""
    n = tops.shape[0]
    p, delta = _ray_samples(tops, bots, tv, S, zero_oob)
    sun = suns.unsqueeze(1).expand(n, S, 3).reshape(-1, 3)
    rho, vis, _ = net.forward_Solar(p.reshape(-1, 3), sun, torch.zeros(n * S, 4, device=tops.device))
    y = rho.detach().reshape(n, S).double() * delta.double()
    vis = vis.detach().reshape(n, S).double()
    c = torch.cumsum(torch.cat([torch.zeros_like(y[:, :1]), y], 1), 1)
    pv = torch.exp(-c[:, :-1])
    ps = pv * (1.0 - torch.exp(-y))
    ex, es = pv > 0.5, vis > 0.5
    d = pv - vis
    return torch.stack([(ex & es).sum(1).double(), ex.sum(1).double(), es.sum(1).double(), (d * d).sum(1), d.abs().sum(1), (ps * vis).sum(1), ps.sum(1),
                        c[:, -1]], 1).float()


def shadow_walk(net, top, bot, sun, S, *, zero_oob=True):
    """The shadow test's per-ray sums for rays top -> bot with one sun direction per ray (`sun` [R,3], passed to the network as given: the reference
    passes its un-normalised sun vector) -> `ShadowWalk`.  S samples at t_s = s / S, every one counting; zero_oob: a sample outside [-1,1]^3 gets
    delta 0 (mg_Shadow_Eval.py:89).

    On a fused bf16x3 model (widths 64 / 256 / 512) in eval mode one launch of `season_nerf::shadow_walk` per chunk: trunk, density head and the solar
    branch with the transmittance scan and the comparison in the kernel, 32 bytes out per ray and no [R,S] array.  Anything else (int8-resolved models,
    a width without a fused kernel, the one-term "bf16" mode, a module in training mode) gets the same eight numbers from `forward_Solar` on the
    sample points and float64 sums: slower, and correct."""
    with torch.no_grad():
        dev = top.device
        top, bot, sun = top.float().contiguous(), bot.float().contiguous(), sun.float().contiguous()
        R = top.shape[0]
        if bot.shape != (R, 3) or sun.shape != (R, 3) or top.dim() != 2:
            raise ValueError(f"shadow_walk: top {tuple(top.shape)}, bot {tuple(bot.shape)} and sun {tuple(sun.shape)} must all be [R,3]")
        tv = sample_parameters_on(dev, S, eval_mode=True)
        out = torch.empty(R, 8, device=dev)
        if _walks(net) and not net.training:
            from .network import _ops
            chunk = 1 << 22
            for i in range(0, R, chunk):
                j = min(R, i + chunk)
                out[i:j] = _ops().shadow_walk(net.device_model(), top[i:j], bot[i:j], sun[i:j], tv, 2 if zero_oob else 0)
        else:
            # sized as ray_surface sizes the layer-wise engine's chunks: ~32 [points x width] fp32 arrays, ~12 GB of workspace
            chunk = min(1 << 16, max(64, int(12e9 / (128.0 * net.layer_width)) // S))
            for i in range(0, R, chunk):
                j = min(R, i + chunk)
                out[i:j] = _shadow_layerwise(net, top[i:j], bot[i:j], sun[i:j], tv, S, zero_oob)
        return ShadowWalk(out, S)


# ------------------------------------------------------------------------------------------------ the reference's call boundary
def _sun_rays(shadow_angles, ground_points, world_center_LLA, W2L_H):
    """Tops, bots [M,G,3] (float64, as mg_Shadow_Eval.py:80-83 forms them before `.float()`) and the un-normalised-by-z sun vectors [M,3]."""
    shadow_angles, ground_points = np.asarray(shadow_angles, dtype=np.float64), np.asarray(ground_points, dtype=np.float64)
    orig = np.array([world_angle_2_local_vec(a[0], a[1], world_center_LLA, W2L_H) for a in shadow_angles], dtype=np.float64).reshape(-1, 3)
    step = orig / orig[:, 2:3]                    # one unit of height per step: the ray reaches z = +1 and z = -1
    g3 = np.zeros([ground_points.shape[0], 3])
    g3[:, :2] = ground_points                     # the ground points stand at z = 0
    return g3[None, :, :] + step[:, None, :], g3[None, :, :] - step[:, None, :], orig


def eval_shadow_data(shadow_net, shadow_angles, ground_points, Z_points, world_center_LLA, W2L_H, max_batch_size, device):
    """mg_Shadow_Eval.py:72-104 -> Results_Vis_Exact [M,G,Z,1], Results_Vis_Est [M,G,Z,1], Results_Sky_Col [M,3] (float64 numpy).  Per-sample arrays are
    what it returns, so it goes by the per-sample kernels: `forward_Solar` on the sample points and `get_PV`, at most max_batch_size points per call."""
    with torch.no_grad():
        dev = torch.device(device)
        tops64, bots64, orig = _sun_rays(shadow_angles, ground_points, world_center_LLA, W2L_H)
        M, G = tops64.shape[0], tops64.shape[1]
        exact, est = np.zeros([M, G, Z_points, 1]), np.zeros([M, G, Z_points, 1])
        sky = np.zeros([M, 3])
        if M == 0:
            return exact, est, sky
        tops, bots, suns = _f32(tops64, dev), _f32(bots64, dev), _f32(orig, dev)
        tv = sample_parameters_on(dev, Z_points, eval_mode=True)
        step = max(int(max_batch_size) // Z_points, 1)
        for i in range(M):
            for j in range(0, G, step):
                k = min(j + step, G)
                p, delta = _ray_samples(tops[i, j:k], bots[i, j:k], tv, Z_points, True)
                n = (k - j) * Z_points
                rho, vis, sky_raw = shadow_net.forward_Solar(p.reshape(-1, 3), suns[i].reshape(1, 3).expand(n, 3), torch.zeros(n, 4, device=dev))
                pv = get_PV(rho.reshape(k - j, Z_points, 1), delta.reshape(k - j, Z_points, 1).contiguous())
                exact[i, j:k] = pv.reshape(k - j, Z_points, 1).cpu().numpy()
                est[i, j:k] = vis.reshape(k - j, Z_points, 1).cpu().numpy()
                if j == 0:
                    sky[i] = sky_raw[0].cpu().numpy()      # the sky network sees the sun direction alone: any row of the call
        return exact, est, sky


def shadow_anaylysis(Ground_Points, Solar_el_az, Results_Dict):
    """mg_Shadow_Eval.py:134-163 on per-sample arrays [M,G,Z,1] (numpy)."""
    ex, es = np.asarray(Results_Dict["Exact_Vis"]), np.asarray(Results_Dict["Est_Vis"])
    d = ex - es
    gt, et = ex > .5, es > .5
    offset = np.abs(gt.sum(2).astype(np.int64) - et.sum(2).astype(np.int64)).mean() if d.size else np.float64("nan")
    return _scores_from_sums(np.sum(gt * et), np.sum(gt), np.sum(et), np.sum(d ** 2), np.sum(np.abs(d)), d.size, offset)


def Test_Shadow_Points(shadow_net, training_points, testing_points, close_walking_points, all_walking_points, ground_points, world_center_LLA, W2L_H,
                       device, Z_points=96, max_batch_size=15000, full_return=True):
    """mg_Shadow_Eval.py:107-131.  full_return=True: the reference's summary with the per-sample arrays of the four sets of sun directions
    (`eval_shadow_data`).  full_return=False: the scores alone, {"Training", "Testing", "Near", "Full"} -> the dict of `shadow_anaylysis`; the rays -
    tops and bots formed in float64 as ground -+ sun_vec / sun_vec_z, cast to float32 - go through `shadow_walk` and no per-sample array is formed."""
    sets = (("Training", training_points), ("Testing", testing_points), ("Near", close_walking_points), ("Full", all_walking_points))
    if not full_return:
        dev = torch.device(device)
        ans = {}
        for name, angles in sets:
            tops64, bots64, orig = _sun_rays(angles, ground_points, world_center_LLA, W2L_H)
            M, G = tops64.shape[0], tops64.shape[1]
            suns = _f32(orig, dev).unsqueeze(1).expand(M, G, 3).reshape(-1, 3)
            ans[name] = shadow_walk(shadow_net, _f32(tops64, dev).reshape(-1, 3), _f32(bots64, dev).reshape(-1, 3), suns, Z_points).scores()
        return ans
    summary = {"Ground_Points": ground_points, "Sun_El_Az": {"Training": training_points, "Testing": testing_points, "Near_Walk": close_walking_points,
                                                             "Full_Walk": all_walking_points}}
    for (name, angles), key in zip(sets, ("Training_Results", "Testing_Results", "Near_Results", "Full_Results")):
        ex, es, sky = eval_shadow_data(shadow_net, angles, ground_points, Z_points, world_center_LLA, W2L_H, max_batch_size, device)
        summary[key] = {"Exact_Vis": ex, "Est_Vis": es, "Sky_Col": sky}
    return summary
