"""season_nerf::loss_terms_all - the fused loss terms of every configuration: MSE or Barron's adaptive colour loss, free or DSM-prior phase
(csrc/train_kernels.hip loss_all_partial_kernel / loss_all_finalize_kernel / loss_all_bwd_kernel) - on the GPU:
  * the kernels through the C ABI against float64 (tests/loss_all_cases.reference: adaptive_loss.py's own functions and torch.autograd in float64 on the
    CPU, alpha and scale as leaves), over the alpha set, NaN sentinels around every output, two launches on the same inputs bit for bit, the albedo
    minima and the rows that own them exactly;
    tolerance train_kernel_cases.tolerance(E_ref, scale) = 4 (E_ref + 2^-24 scale), E_ref = the float32 evaluation of the same reference on these inputs;
  * the op and its registered backward inside a training step against the tensor-op path of get_loss;
  * the captured step under fused_loss="all" against the eager one, its graph's nodes;
  * fused_loss="default" and SNERF_FUSED_LOSS=0 reach the code they reached before."""
import ctypes as C
import glob
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import loss_all_cases as lc
import train_kernel_cases as tk

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WC, H4 = np.array([41.29, -95.9, 300.0]), np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])
# one ray | odd sizes | > 64 blocks for the finalize wave | R S past the 1024-block cap | the image rays past it (262200 elements) | the sun rays past it
SIZES = [(1, 1, 1), (257, 131, 7), (5547, 300, 40), (3000, 1000, 96), (87400, 1000, 13), (1000, 10925, 30)]
SIZE_IDS = ["one-ray", "R257", "blocks-over-64", "RS-over-1024-blocks", "R87400-over-1024-blocks", "sun-rays-over-1024-blocks"]
PAD = 16


@pytest.fixture(scope="module")
def L():
    import season_nerf_amd as sn
    return sn._lib.lib()


def _guarded(shape):
    """an output inside a NaN-filled buffer -> (buffer, the output's view)"""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), float("nan"), device="cuda")
    return buf, buf[PAD:PAD + n].view(*shape)


def _pads_untouched(buf):
    return bool(torch.isnan(buf[:PAD]).all()) and bool(torch.isnan(buf[-PAD:]).all())


def _ratio(err, tol):
    return float(np.max(np.where(err == 0, 0, err / np.maximum(tol, 1e-300))))


@pytest.mark.parametrize("config", list(lc.CONFIGS))
@pytest.mark.parametrize("R,Rs,S", SIZES, ids=SIZE_IDS)
def test_loss_all_kernels_against_float64(L, R, Rs, S, config):
    from season_nerf_amd._lib import LossIn, LossGrads
    from season_nerf_amd.adaptive_loss import table_on
    flags = lc.CONFIGS[config]
    ada, prior = bool(flags & lc.ADAPTIVE), bool(flags & lc.PRIOR)
    names = lc.NAMES[flags & 3]
    n = len(names)
    assert L.snerf_loss_all_term_count(flags) == n
    p = lambda t: t.data_ptr() if t is not None else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    scratch = torch.full((L.snerf_loss_all_scratch_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")      # no initial state needed: garbage will do
    lz_v, lz_s = table_on("cuda:0", torch.float64)
    g = np.linspace(0.5, 1.5, n).astype(np.float32)
    worst = {}
    for alpha in (lc.ALPHAS if ada else lc.ALPHAS[:1]):                  # (the MSE configurations read no alpha)
        h = lc.make_inputs(f"loss-all-{R}-{Rs}-{S}", R, Rs, S, alpha)
        v64, w64, scale, g64 = lc.reference(h, flags, torch.float64, g)
        v32, w32, _, g32 = lc.reference(h, flags, torch.float32, g)
        dev = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in h.items() if k != "w"}
        i = LossIn(n_rays=R, n_solar_rays=Rs, n_samples=S, flags=flags, world=1, w_solar=h["w"][0], w_color=h["w"][1], w_alpha=h["w"][2])
        i.d_rgb, i.d_gt, i.d_albedo, i.d_sky = p(dev["rgb"]), p(dev["gt"]), p(dev["albedo"]), p(dev["sky"])
        i.d_rgb_merged = p(dev["rgb_merged"]) if prior else None
        i.d_solar_vis, i.d_pv_exact, i.d_pe_solar = p(dev["sv"]), p(dev["pv"]), p(dev["pe_sun"])
        if prior:
            i.d_pe, i.d_pe_supervised = p(dev["pe"]), p(dev["pe_sup"])
        if ada:
            i.d_alpha_color, i.d_scale_color, i.d_logz_value, i.d_logz_slope = p(dev["alpha_c"]), p(dev["scale_c"]), p(lz_v), p(lz_s)
            if prior:
                i.d_alpha_alpha, i.d_scale_alpha = p(dev["alpha_a"]), p(dev["scale_a"])
        first = None
        for rep in range(2):
            fb = [_guarded((n,)), _guarded((n,)), _guarded((14,))]
            rc = L.snerf_loss_all_forward(C.byref(i), p(scratch), p(fb[0][1]), p(fb[1][1]), p(fb[2][1]), st)
            assert rc == 0, L.snerf_last_error().decode()
            shapes = {"rgb": (R, 3), "rgb_merged": (R, 3) if prior else None, "albedo": (R, 3), "sky": (R, 3), "sv": (Rs, S), "pe": (R, S) if prior else None,
                      "alpha_c": (3,) if ada else None, "scale_c": (3,) if ada else None, "alpha_a": (1,) if ada and prior else None,
                      "scale_a": (1,) if ada and prior else None}
            gb = {k: (_guarded(s) if s is not None else (None, None)) for k, s in shapes.items()}
            gd = torch.from_numpy(g).cuda()
            o = LossGrads(*[p(gb[k][1]) for k in ("rgb", "rgb_merged", "albedo", "sky", "sv", "pe", "alpha_c", "scale_c", "alpha_a", "scale_a")])
            rc = L.snerf_loss_all_backward(C.byref(i), p(fb[2][1]), p(gd), C.byref(o), st)
            assert rc == 0, L.snerf_last_error().decode()
            torch.cuda.synchronize()
            for buf, _ in fb + [b for b in gb.values() if b[0] is not None]:
                assert _pads_untouched(buf)
            bits = [t[1].clone() for t in fb] + [gb[k][1].clone() for k in gb if gb[k][0] is not None]
            if first is None:
                first = bits
            else:                                                        # no floating-point atomics: the same bits from launch to launch
                for a_, b_ in zip(first, bits):
                    assert torch.equal(a_.view(torch.int32), b_.view(torch.int32))
        vals, wts = fb[0][1].cpu().numpy().astype(np.float64), fb[1][1].cpu().numpy().astype(np.float64)
        aux = fb[2][1].cpu().numpy()
        np.testing.assert_array_equal(aux[:3], h["albedo"].min(0))                       # the float32 column minima, exactly
        np.testing.assert_array_equal(aux[3:6].view(np.int32), h["albedo"].argmin(0))    # the lowest row that attains each
        assert ada or not aux[6:].any()
        for what, got, want, e_ref, sc in (("vals", vals, v64, np.abs(v32 - v64), scale), ("weights", wts, w64, np.abs(w32 - w64), np.abs(w64))):
            tol = tk.tolerance(e_ref, sc)
            err = np.abs(got - want)
            worst[what] = max(worst.get(what, 0), _ratio(err, tol))
            assert (err <= tol).all(), (alpha, what, names, got, want, tol)
        for k, (buf, out) in gb.items():
            if buf is None:
                continue
            got = out.cpu().numpy().astype(np.float64)
            if g64[k] is None:                                           # a value only in this configuration: the gradient is written as zeros
                assert not got.any(), (alpha, k)
                continue
            want, w32_ = g64[k].reshape(got.shape), g32[k].reshape(got.shape)
            e_ref = float(np.abs(w32_ - want).max())
            tol = tk.tolerance(e_ref, np.abs(want))
            err = np.abs(got - want)
            worst["d_" + k] = max(worst.get("d_" + k, 0), _ratio(err, tol))
            assert (err <= tol).all(), (alpha, k, float(err.max()), e_ref, got.reshape(-1)[:4], want.reshape(-1)[:4])
    print(f"FIG loss_all {config} R={R} Rs={Rs} S={S}: worst deviation / tolerance " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))


# ------------------------------------------------------------------------------------------------------------------ the op inside a training step
STEP_CONFIGS = {"adaptive-free": (False, False), "adaptive-prior": (False, True), "mse-prior": (True, True)}      # (Use_MSE_loss, DSM prior)


def _setup(use_mse, prior, fused_loss, W=64, R=32, S=32, seed=5):
    import season_nerf_amd as sn
    from oracle import season_nerf_oracle as orc
    from season_nerf_amd.adaptive_loss import AdaptiveLossFunction
    hm = np.random.Generator(np.random.PCG64(3)).uniform(-0.8, 0.6, (24, 24))
    rng = np.random.Generator(np.random.PCG64(seed))
    t = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")
    sun = rng.uniform(0.1, 1, (R, 3)); sun /= np.linalg.norm(sun, axis=1, keepdims=True)
    tau = rng.uniform(0, 1, (R, 2))
    data = {"Top": t(np.concatenate([rng.uniform(-1, 1, (R, 2)), np.ones((R, 1))], 1)), "Bot": t(np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1)),
            "Sun_Angle": t(sun), "Time_Encoded": t(np.stack([np.cos(6.28 * tau[:, 0]), np.sin(6.28 * tau[:, 0]), np.cos(6.28 * tau[:, 1]), np.sin(6.28 * tau[:, 1])], 1)),
            "GT_Color": t(rng.uniform(0, 1, (R, 3)))}
    net = sn.T_NeRF(W, 4, HM=hm) if prior else sn.T_NeRF(W, 4)
    net.load_state_dict(orc.init_weights(W, 4, 7, bn_stats="identity"))
    net = net.cuda().train()
    args = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=use_mse, Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=4)
    mk = lambda dims, a0, s0, slo: AdaptiveLossFunction(dims, torch.float32, "cuda", alpha_hi=2.99, alpha_init=a0, scale_init=s0, scale_lo=slo)
    ada = None if use_mse else ([mk(3, 2.0, .03, .01), mk(1, 2.0, .5, .05)] if prior else mk(3, 2.0, .03, .01))       # as Net_Tool_2.py:69-82 builds them
    ev = sn.All_in_One_Eval(args, torch.device("cuda"), 40, prior, ada, H4, WC)       # a 40-step phase: the prior's trust factor step / 40 stays below 1 over the 20 steps run here
    ev.fused_loss = fused_loss
    return sn, net, ev, data, ada


def _terms_float64(ev, net, data, step):
    """training.get_loss's tensor-op path (Eval_Tools_2.py:340-459) with every term formed in float64 from the passes' float32 outputs: the yardstick that
    says what float32 arithmetic in the loss terms costs the gradients of this step"""
    from season_nerf_amd import adaptive_loss as al
    from season_nerf_amd.training import albedo_min_loss
    args = ev.args
    d = lambda x: x.double()
    sq = lambda x: x * x
    mse = lambda a, b: torch.mean(sq(a - b))
    out = ev.eval(data, net, step, True)
    starts, ends, vec, stime, _ = ev.solar_creation_tool(data["Top"].shape[0], include_times=True)
    so = ev.eval_Rho_Only({"Top": starts, "Bot": ends, "Sun_Angle": vec, "Time_Encoded": stime}, net, True, step)
    w = args.sc_lambda
    Loss = {}
    Loss["Solar_Correction"] = [torch.mean(torch.sum(sq(d(so["Solar_Vis"]) - d(so["PV_Exact"]).detach()), 1)), w]
    Loss["Solar_Correction_2"] = [torch.mean(1 - torch.sum(d(so["PE"]).detach() * d(so["PV_Exact"]).detach() * d(so["Solar_Vis"]), 1)).detach(), w]
    x = (d(out["Sky_Col"]) - .5) / .5
    sk = torch.sum(torch.where(x > 0, sq(x), torch.zeros_like(x))) / x.numel()
    Loss["Sky_Color_Var"] = [sk.detach() if ev.use_prior else sk, w]
    Loss["Albedo_Color"] = [albedo_min_loss(d(out["Albedo_Color"])), w]
    gt = d(data["GT_Color"])
    col = d(out["Rendered_Col_Merged"] if ev.use_prior else out["Rendered_Col"])
    nll = lambda m, x_: al.general_loss(x_, d(m.alpha()), d(m.scale())) + torch.log(d(m.scale())) + al.log_base_partition_function(d(m.alpha()))
    if ev.use_MSE_loss:
        Loss["Color"] = [mse(col, gt), 1.0]
        Loss["Alpha_Adjust"] = [mse(d(out["PE"]), d(out["PE_Supervised"]).detach()), 1.]
    else:
        ada = ev.ada_loss[0] if ev.use_prior else ev.ada_loss
        if ev.use_prior:
            Loss["Alpha_Adjust_ada"] = [torch.mean(nll(ev.ada_loss[1], (d(out["PE"]) - d(out["PE_Supervised"]).detach()).reshape(-1, 1))), 1.]
        Loss["Color_ada"] = [torch.mean(nll(ada, d(out["Rendered_Col"]) - gt)), 1.0]
        Loss["Color_alpha"], Loss["Color_width"] = [torch.mean(d(ada.alpha()).detach()), 1.], [torch.mean(d(ada.scale()).detach()), 1.]
        if ev.use_prior:
            Loss["Alpha_Adjust"] = [mse(d(out["PE"]), d(out["PE_Supervised"]).detach()), 1.]
        s2 = torch.mean(d(ada.scale()).detach()) ** 2
        Loss["Solar_Correction"][1], Loss["Solar_Correction_2"][1] = w / s2, w / s2
        if ev.use_prior:
            Loss["Alpha_alpha"], Loss["Alpha_width"] = [torch.mean(d(ev.ada_loss[1].alpha()).detach()), 1.], [torch.mean(d(ev.ada_loss[1].scale()).detach()), 1.]
        Loss["Color"] = [mse(col, gt).detach(), 1.0]
    return Loss


def _one_step(use_mse, prior, mode):
    """one forward + backward of the step's loss -> ({name: (value, weight)} as floats, key order, {tensor name: gradient}, the returned dict)"""
    sn, net, ev, data, ada = _setup(use_mse, prior, "all" if mode == "all" else "default")
    np.random.seed(11); torch.manual_seed(11)
    loss = _terms_float64(ev, net, data, 3) if mode == "float64" else ev.get_loss(data, net, 3, True)
    total = loss.total() if getattr(loss, "vec", None) is not None else sum(v[0] * v[1] for v in loss.values())
    total.backward()
    torch.cuda.synchronize()
    grads = {k: p_.grad.detach().double().cpu().clone() for k, p_ in net.named_parameters() if p_.grad is not None}
    mods = [] if ada is None else (ada if isinstance(ada, list) else [ada])
    for j, m in enumerate(mods):
        grads[f"ada{j}.latent_alpha"], grads[f"ada{j}.latent_scale"] = m.latent_alpha.grad.double().cpu().clone(), m.latent_scale.grad.double().cpu().clone()
    vals = {k: (float(v[0]), float(v[1])) for k, v in loss.items()}
    return vals, list(loss.keys()), grads, loss


@pytest.mark.parametrize("config", list(STEP_CONFIGS))
def test_op_against_the_tensor_op_path(config):
    """One training step at W = 64, R = 32, S = 32: values, weights and key order of get_loss under "all" equal those under "default"; the gradients of every
    network parameter and of the loss objects' latents lie within 4 (D + 2^-24 largest magnitude) of the default path's, D = the distance between the default
    path's gradients and the same step with its loss terms formed in float64 tensor ops (the yardstick is the tensor-op path, not the new kernels)."""
    from season_nerf_amd.training import LossDict
    use_mse, prior = STEP_CONFIGS[config]
    va, ka, ga, la = _one_step(use_mse, prior, "default")
    vb, kb, gb, _ = _one_step(use_mse, prior, "float64")
    vc, kc, gc, lc_ = _one_step(use_mse, prior, "all")
    assert not isinstance(la, LossDict) and isinstance(lc_, LossDict) and lc_.wvec is not None
    assert ka == kb == kc == list(lc.NAMES[(0 if use_mse else 1) | (2 if prior else 0)]) == list(lc_.names)
    for k in ka:
        for j, what in enumerate(("value", "weight")):
            D = abs(va[k][j] - vb[k][j])
            bound = 4 * (D + 2.0 ** -24 * abs(va[k][j]))
            print(f"FIG {config} {k} {what}: default {va[k][j]:.8g} all {vc[k][j]:.8g} float64 {vb[k][j]:.8g} |all - default| / bound {abs(vc[k][j] - va[k][j]) / max(bound, 1e-300):.3f}")
            assert abs(vc[k][j] - va[k][j]) <= bound, (k, what, va[k], vc[k], vb[k])
        assert torch.is_tensor(lc_[k][1]) == torch.is_tensor(la[k][1]), k               # tensor weights for the two scaled terms, floats elsewhere
    assert set(ga) == set(gb) == set(gc) and (use_mse or any(k.startswith("ada") for k in ga))
    worst = ("", 0.0)
    for k in ga:
        D = float((ga[k] - gb[k]).abs().max())
        bound = 4 * (D + 2.0 ** -24 * float(ga[k].abs().max()))
        err = float((gc[k] - ga[k]).abs().max())
        if err > worst[1] * max(bound, 1e-300):
            worst = (k, err / max(bound, 1e-300))
        assert err <= bound, (k, err, D, float(ga[k].abs().max()))
    print(f"FIG {config}: {len(ga)} gradient tensors, worst |all - default| / bound {worst[1]:.3f} at {worst[0]}")


def test_op_checks_and_data_parallel_inputs():
    """torch.library.opcheck on both new ops; the data-parallel inputs (albedo_min_global, world = 2) as test_fused_loss_terms_vs_tensor_ops covers them"""
    import season_nerf_amd as sn
    from season_nerf_amd import training
    from season_nerf_amd.adaptive_loss import table_on
    sn.ops.load()
    training._register_autograd()
    R, Rs, S = 64, 48, 40
    h = lc.make_inputs("op-dp", R, Rs, S, 1.3)
    T = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in h.items() if k != "w"}
    for k in ("alpha_c", "scale_c", "alpha_a", "scale_a"):
        T[k] = T[k].reshape(1, -1)
    lz_v, lz_s = table_on(T["rgb"].device, torch.float64)
    args = lambda g_min, world, flags: (T["rgb"], T["rgb_merged"], T["gt"], T["albedo"], T["sky"], T["sv"].unsqueeze(-1), T["pv"].unsqueeze(-1), T["pe_sun"].unsqueeze(-1),
                                        T["pe"].unsqueeze(-1), T["pe_sup"].unsqueeze(-1), T["alpha_c"], T["scale_c"], T["alpha_a"], T["scale_a"], lz_v, lz_s, g_min, world,
                                        flags, 0.03, 1.0, 1.0)
    for flags in (1, 7, 6):
        torch.library.opcheck(torch.ops.season_nerf.loss_terms_all.default, args(None, 1, flags), test_utils=("test_schema", "test_faketensor"))
        vals, wts, aux = torch.ops.season_nerf.loss_terms_all(*args(None, 1, flags))
        a = args(None, 1, flags)
        torch.library.opcheck(torch.ops.season_nerf.loss_terms_all_bwd.default, (torch.ones_like(vals), a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[8], a[9], a[10], a[11],
                                                                                 a[12], a[13], aux, flags), test_utils=("test_schema", "test_faketensor"))
    albedo = T["albedo"].clone().requires_grad_(True)
    T["albedo"] = albedo
    g_min = albedo.detach().min(0).values * torch.tensor([1.0, 0.5, 1.0], device="cuda")        # another rank owns channel 1's minimum
    vals, wts, aux = torch.ops.season_nerf.loss_terms_all(*args(g_min, 2, 7))
    hinge = torch.sum(torch.where(g_min < .2, (1 - g_min / .2) ** 2, torch.zeros_like(g_min))) / (2 * R)
    np.testing.assert_allclose(float(vals[3]), float(hinge), rtol=2e-6)
    vals[3].backward()
    assert bool((albedo.grad[:, 1] == 0).all()) and int((albedo.grad[:, 0] != 0).sum()) == 1 and int((albedo.grad[:, 2] != 0).sum()) == 1
    with pytest.raises(RuntimeError, match="prior phase needs"):
        torch.ops.season_nerf.loss_terms_all(T["rgb"], None, T["gt"], albedo.detach(), T["sky"], T["sv"], T["pv"], T["pe_sun"], None, None, None, None, None, None, None, None,
                                             None, 1, 2, 0.03, 1.0, 1.0)


# ------------------------------------------------------------------------------------------------------------------ the captured step
def _run_steps(use_mse, prior, graphed, n_steps=20):
    sn, net, ev, data, ada = _setup(use_mse, prior, "all", R=48)
    tool = sn.Net_tool(net, ev, 3e-4, total_steps=n_steps + 1, lr_alpha_scale=30.0, writer=None)
    step = sn.GraphedTrainStep(tool, data, warmup=2) if graphed else None
    ada0 = [p_.detach().clone() for p_ in tool._ada_params]
    np.random.seed(11); torch.manual_seed(11)
    losses = []
    for k in range(n_steps):
        loss = step(data, k) if graphed else tool.train_step(data, k)
        assert getattr(loss, "wvec", None) is not None
        losses.append({n: float(v[0]) for n, v in loss.items()})
    if graphed:
        assert step.graph is not None and step.calls == n_steps and step.disabled is None
    return losses, {k: v.detach().clone() for k, v in net.state_dict().items()}, [(p_.detach().clone(), p0) for p_, p0 in zip(tool._ada_params, ada0)]


@pytest.mark.parametrize("config", list(STEP_CONFIGS))
def test_captured_step_under_all_follows_the_eager_step(config):
    """20 steps under fused_loss="all", captured against eager, in the band of tests/test_net_tool.py::test_graphed_train_step_follows_the_eager_step: loss values
    to 2e-4, the loss objects' latents to 3 % of the distance they travelled, the parameters to 2 % of the distance travelled."""
    from oracle import season_nerf_oracle as orc
    use_mse, prior = STEP_CONFIGS[config]
    le, pe, ae = _run_steps(use_mse, prior, False)
    lg, pg, ag = _run_steps(use_mse, prior, True)
    assert len(ae) == (0 if use_mse else (4 if prior else 2))
    for (a, a0), (b, _) in zip(ae, ag):
        moved = float((a - a0).abs().max())
        assert moved > 1e-3 and float((a - b).abs().max()) <= 0.03 * moved, (a0, a, b)
    for k in range(len(le)):
        for n, v in le[k].items():
            assert abs(lg[k][n] - v) <= 2e-4 * max(abs(v), 1e-3), (k, n, lg[k][n], v)
    p0 = orc.init_weights(64, 4, 7, bn_stats="identity")
    moved = diff = 0.0
    for k, v in pe.items():
        if v.is_floating_point() and "running" not in k:
            moved += float((v.cpu() - p0[k]).abs().sum())
            diff += float((pg[k] - v).abs().sum())
        elif not v.is_floating_point():
            assert torch.equal(pg[k], v), k
    print(f"FIG {config}: graphed vs eager after 20 steps: sum |difference| / sum |update| = {diff / moved:.2e}")
    assert moved > 0 and diff < 0.02 * moved, (diff, moved)


CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, torch
import season_nerf_amd as sn
from test_gpu_loss_all import _setup, STEP_CONFIGS
use_mse, prior = STEP_CONFIGS[%r]
for mode in ("all", "default"):
    os.makedirs(mode)
    os.chdir(mode)                                      # the runtime prints a captured graph into the working directory
    sn_, net, ev, data, ada = _setup(use_mse, prior, mode, R=48)
    tool = sn.Net_tool(net, ev, 3e-4, total_steps=8, lr_alpha_scale=30.0, writer=None)
    step = sn.GraphedTrainStep(tool, data, warmup=2)
    for k in range(4):
        loss = step(data, k)
    torch.cuda.synchronize()
    print(mode, "replayed", int(step.graph is not None), type(loss).__name__, getattr(loss, "wvec", None) is not None, flush=True)
    os.chdir("..")
"""


def _graph_labels(tmp_path, config):
    """one child process captures the step under "all" and under "default" -> the node labels of both graphs"""
    env = dict(os.environ, DEBUG_HIP_GRAPH_DOT_PRINT="1")
    env.pop("SNERF_TRAIN_MEMOPS", None)
    env.pop("SNERF_FUSED_LOSS", None)
    r = subprocess.run([sys.executable, "-c", CHILD % (REPO, REPO, config)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "all replayed 1 LossDict True" in r.stdout and "default replayed 1" in r.stdout and "default replayed 1 LossDict True" not in r.stdout, r.stdout
    labels = []
    for mode in ("all", "default"):
        dots = sorted(glob.glob(os.path.join(str(tmp_path), mode, "graph_*dot_print*")))
        assert len(dots) == 1, (mode, dots, r.stderr[-500:])
        labels.append(re.findall(r'label="\d+\n([^\n"]*)', open(dots[0]).read()))
    return labels


@pytest.mark.parametrize("config", list(STEP_CONFIGS))
def test_captured_step_under_all_holds_kernel_nodes_only_and_fewer_of_them(tmp_path, config):
    """The runtime's own DOT print of the captured step (a child process: the switch is read at HIP start-up): kernel nodes only under "all", the three loss
    kernels among them, and strictly fewer nodes than the same step under "default".  Measured on an MI355X (nodes under "all" / "default"): adaptive loss,
    free phase 281 / 514; adaptive loss, prior phase 338 / 740; MSE loss, prior phase 284 / 347."""
    all_, dflt = _graph_labels(tmp_path, config)
    print(f"FIG {config}: captured step holds {len(all_)} nodes under 'all', {len(dflt)} under 'default'")
    memops = [l for l in all_ if re.search(r"memcpy|memset", l, re.I)]
    assert not memops, sorted(set(memops))
    for kern in ("loss_all_partial_kernel", "loss_all_finalize_kernel", "loss_all_bwd_kernel"):
        assert sum(kern in l for l in all_) == 1, kern
        assert not any(kern in l for l in dflt), kern
    assert 100 < len(all_) < len(dflt)


# ------------------------------------------------------------------------------------------------------------------ default behaviour
def test_default_and_switch_reach_the_code_they_reached(monkeypatch):
    """fused_loss="default" (and the keyword's default) keeps every configuration where it was: the generic dict for the adaptive loss and the prior phase, the
    fused op for the MSE free phase - whose loss vector is, bit for bit, what season_nerf::loss_terms_all at flags 0 gives on the step's tensors (the sums
    are reproducible), under "all" too; and SNERF_FUSED_LOSS=0 turns every fused path off, "all" included."""
    import season_nerf_amd as sn
    from season_nerf_amd import training
    from season_nerf_amd.training import LossDict
    assert sn.All_in_One_Eval.fused_loss == "default"
    with pytest.raises(ValueError, match="fused_loss"):
        sn.T_NeRF_Net_Tool(SimpleNamespace(max_train_steps=10), None, None, "cuda", H4, WC, fused_loss="some")
    for use_mse, prior in STEP_CONFIGS.values():
        _, net, ev, data, _ = _setup(use_mse, prior, "default")
        with torch.no_grad():
            loss = ev.get_loss(data, net, 3, True)
        assert type(loss) is dict
        monkeypatch.setenv("SNERF_FUSED_LOSS", "0")
        ev.fused_loss = "all"
        with torch.no_grad():
            assert type(ev.get_loss(data, net, 3, True)) is dict
        monkeypatch.delenv("SNERF_FUSED_LOSS")
    seen = {}
    orig = training._fused_loss

    def spy(ev_, net_, out, so, gt, weight, train_mode):
        seen["args"] = (out["Rendered_Col"], None, gt.contiguous(), out["Albedo_Color"], out.sky_ray, so["Solar_Vis"], so["PV_Exact"].detach(), so["PE"].detach())
        return orig(ev_, net_, out, so, gt, weight, train_mode)

    monkeypatch.setattr(training, "_fused_loss", spy)
    for mode in ("default", "all"):
        _, net, ev, data, _ = _setup(True, False, mode)
        with torch.no_grad():
            loss = ev.get_loss(data, net, 3, True)
            assert isinstance(loss, LossDict) and loss.wvec is None and loss.names == ("Solar_Correction", "Solar_Correction_2", "Sky_Color_Var", "Albedo_Color", "Color")
            want = torch.ops.season_nerf.loss_terms_all(*seen.pop("args"), *[None] * 9, 1, 0, 0.03, 1.0, 1.0)[0]
        assert torch.equal(loss.vec.view(torch.int32), want.view(torch.int32))
        monkeypatch.setenv("SNERF_FUSED_LOSS", "0")
        with torch.no_grad():
            assert type(ev.get_loss(data, net, 3, True)) is dict and "args" not in seen
        monkeypatch.delenv("SNERF_FUSED_LOSS")
