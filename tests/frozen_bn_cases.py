"""Cases, inputs and float64 references for the training engine's backward after a forward with frozen BatchNorm (train_bn = 0: the running
statistics normalise, nothing is updated).  Shared by tests/test_gpu_train_frozen_bn.py (the engine against these references on the GPU) and
tests/test_frozen_bn_refs.py (the references against torch.nn.BatchNorm1d.eval() and the conditions that keep the case list honest, on the CPU).

Reference: the oracle with train_bn=False on orc.cast_weights(sd, float64), requires_grad on every floating-point entry but the running statistics
(the oracle would hand those a gradient; a module holds them as buffers).  Inputs are seeded fp32 tensors; the reference gets the same values cast to
float64.  Every float64 reference is computed once per process and shared (reference()).

Weights: orc.init_weights(W, C, seed, bn_stats="random") with every BatchNorm gamma redrawn from U(0.5, 1.5) and every beta from U(-0.3, 0.3): neither
the folded scale gamma istd nor the shift is trivial.

Sizes follow the engine's routing (csrc/linear_product.h, rows_min = 1024): 12 rays x 16 samples = 192 points take the fp32 route (colreduce mode 1,
then a bn_bwd2 pass of its own); 33 x 37 = 1221 points (and 35 x 33 = 1155) the row-GEMM route, ragged against the 32-, 256- and 512-row tiles:
activation on load with the table built from the running statistics, the activation backward in the dgrad epilogue, the BatchNorm dZ riding in the
weight-gradient kernel.

Gradient error, as tests/test_gpu_train.py::test_ragged_batch_vs_oracle takes it: per tensor max|got - ref64| / max(max|ref64|, 1e-3 gmax), gmax the
largest float64 gradient of the case; BAR = 2e-3 is that test's bar.
"""
import contextlib
from collections import namedtuple

import numpy as np
import torch

from oracle import season_nerf_oracle as orc

BAR = 2e-3
SC_LAMBDA = 0.03

# kind: "image" (op level: train_fwd_image + compositing), "points" (train_fwd_points), "solar" (train_fwd_solar; its backward meets no BatchNorm
# layer: the control), "seam" (All_in_One_Eval.get_loss on a module in .eval())
Case = namedtuple("Case", "id kind W C R S classic seed")
CASES = [
    Case("image_W64_12x16", "image", 64, 4, 12, 16, False, 21),
    Case("image_W64_33x37", "image", 64, 4, 33, 37, False, 22),
    Case("image_W256_12x16", "image", 256, 4, 12, 16, False, 23),
    Case("image_W256_33x37", "image", 256, 4, 33, 37, False, 24),
    Case("image_W512_35x33", "image", 512, 4, 35, 33, False, 25),          # the gemm_areg form of the activation backward
    Case("image_W64_33x37_classic", "image", 64, 4, 33, 37, True, 26),     # the solar branch feeds dX1: another dgrad does fc9's activation backward
    Case("points_W64_1221", "points", 64, 4, 1221, 1, False, 27),
    Case("solar_W64_12x16", "solar", 64, 4, 12, 16, False, 28),
    Case("solar_W64_33x37", "solar", 64, 4, 33, 37, False, 29),
    Case("seam_W128_35x33", "seam", 128, 4, 35, 33, False, 30),
    Case("seam_W100_35x33", "seam", 100, 4, 35, 33, False, 31),            # not a multiple of 16: no activation on load
]
BY_ID = {c.id: c for c in CASES}


def T(a):
    return torch.tensor(np.asarray(a), dtype=torch.float32)


def weights(case):
    """fp32 state dict of the case: random running statistics, perturbed BatchNorm affine"""
    sd = orc.init_weights(case.W, case.C, case.seed, bn_stats="random")
    rng = np.random.Generator(np.random.PCG64(1000 + case.seed))
    for k in sorted(sd):
        if k.endswith(".norm.weight"):
            sd[k] = T(rng.uniform(0.5, 1.5, sd[k].shape))
        elif k.endswith(".norm.bias"):
            sd[k] = T(rng.uniform(-0.3, 0.3, sd[k].shape))
    return sd


def inputs(case):
    """Seeded fp32 inputs: the ray batch (or points), the sun-ray batch, and the weights of the linear functional that serves as the loss."""
    rng = np.random.Generator(np.random.PCG64(2000 + case.seed))
    R, S, C = case.R, case.S, case.C
    sun = rng.uniform(0.1, 1, (R, 3)); sun /= np.linalg.norm(sun, axis=1, keepdims=True)
    tau = rng.uniform(0, 1, (R, 2))
    tim = np.stack([np.cos(6.28 * tau[:, 0]), np.sin(6.28 * tau[:, 0]), np.cos(6.28 * tau[:, 1]), np.sin(6.28 * tau[:, 1])], 1)
    d = {"Top": T(np.concatenate([rng.uniform(-1, 1, (R, 2)), np.ones((R, 1))], 1)),
         "Bot": T(np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1)), "Sun_Angle": T(sun), "Time_Encoded": T(tim),
         "GT_Color": T(rng.uniform(0, 1, (R, 3)))}
    st = np.concatenate([rng.uniform(-1, 1, (R, 2)), np.ones((R, 1))], 1)
    solar = {"Top": T(st), "Bot": T(st - 2 * sun / sun[:, 2:]), "Sun_Angle": T(sun)}
    X = T(rng.uniform(-1, 1, (R, 3)))                                     # "points": R points
    n = lambda *shape: T(rng.normal(size=shape))
    w = {"image": {"Rendered_Col": n(R, 3), "Albedo_Color": n(R, 3), "Sky_Col": n(R, 3), "PE": n(R, S, 1)},
         "points": {"Rho": n(R, 1), "Col": n(R, 3), "Solar_Vis": n(R, 1), "Sky_Col": n(R, 3), "Classes": n(R, C)},
         "solar": {"Solar_Vis": n(R, S, 1)}, "seam": {}}[case.kind]
    return {"data": d, "solar": solar, "X": X, "w": w}


def cast_inputs(inp, dtype):
    c = lambda v: {k: t.to(dtype) for k, t in v.items()} if isinstance(v, dict) else v.to(dtype)
    return {k: c(v) for k, v in inp.items()}


def is_param(k, v):
    return torch.is_tensor(v) and v.is_floating_point() and "running_" not in k


def run_oracle(case, dtype, sd=None, inp=None):
    """The case on the oracle with frozen BatchNorm in `dtype` -> {"loss", "out": detached outputs, "grads": name -> gradient (None: no path)}."""
    sd = weights(case) if sd is None else sd
    p = {k: (v.to(dtype).clone().requires_grad_(True) if is_param(k, v) else (v.to(dtype) if v.is_floating_point() else v)) for k, v in sd.items()}
    i = cast_inputs(inputs(case) if inp is None else inp, dtype)
    R, S = case.R, case.S
    if case.kind == "image":
        out = orc.eval_rays(p, i["data"], S, train_mode=False, classic_solar=case.classic, train_bn=False)
        out = dict(out, Sky_Col=out["Sky_Col"][:, 0, :])                    # one sky colour per ray, as the engine returns it
        loss = sum((out[k] * w).sum() for k, w in i["w"].items())
    elif case.kind == "points":
        rho, col, sv, sky, cls, adjc = orc.forward(p, i["X"], i["data"]["Sun_Angle"], i["data"]["Time_Encoded"], train_bn=False)
        out = {"Rho": rho, "Col": col, "Solar_Vis": sv, "Sky_Col": sky, "Classes": cls, "Adjust_col": adjc}
        loss = sum((out[k] * w).sum() for k, w in i["w"].items())
    elif case.kind == "solar":
        out = orc.eval_rho_only(p, i["solar"], S, train_mode=False, train_bn=False)
        out = {k: out[k] for k in ("Solar_Vis", "PV_Exact", "PE", "Rho")}
        loss = sum((out[k] * w).sum() for k, w in i["w"].items())
    else:
        terms, out = orc.get_loss_mse(p, i["data"], i["solar"], S, SC_LAMBDA, train_mode=False, train_bn=False)
        loss = orc.total_loss(terms)
        out = dict(out, Sky_Col=out["Sky_Col"][:, 0, :], **{"loss_" + k: v for k, (v, _) in terms.items()})
    loss.backward()
    return {"loss": float(loss.detach()), "out": {k: v.detach() for k, v in out.items() if torch.is_tensor(v)},
            "grads": {k: v.grad for k, v in p.items() if torch.is_tensor(v) and v.requires_grad}}


_REF = {}


def reference(case):
    """the float64 reference of the case, computed once"""
    if case.id not in _REF:
        _REF[case.id] = run_oracle(case, torch.float64)
    return _REF[case.id]


def live(ref):
    """the tensors whose float64 gradient is non-zero, and the largest gradient of the case"""
    names = [k for k, g in ref["grads"].items() if g is not None and float(g.abs().max()) > 0]
    return names, max(float(ref["grads"][k].abs().max()) for k in names)


def grad_errors(got, ref):
    """name -> max|got - ref64| / max(max|ref64|, 1e-3 gmax) over every live tensor; a missing gradient counts as zero"""
    names, gmax = live(ref)
    err = {}
    for k in names:
        r = ref["grads"][k]
        g = got.get(k)
        g = torch.zeros_like(r) if g is None else g.detach().cpu().double()
        err[k] = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-3 * gmax)
    return err


def worst(err):
    k = max(err, key=err.get)
    return err[k], k


# ---- the rule the engine applied before it knew the mode: the batch-statistics backward on running statistics -------------------------------------
class _BatchRuleOnRunningStats(torch.autograd.Function):
    """forward: y = gamma (z - rm) / sqrt(rv + eps) + beta (frozen BatchNorm);  backward: dz = gamma istd (dy - mean(dy) - xhat mean(dy xhat)),
    the derivative of batch-statistics BatchNorm; d gamma = sum dy xhat and d beta = sum dy (right in both modes)."""

    @staticmethod
    def forward(ctx, z, gamma, beta, rm, rv):
        std = torch.sqrt(rv + orc.BN_EPS)
        xhat, istd = (z - rm) / std, 1.0 / std
        ctx.save_for_backward(xhat, gamma, istd)
        return xhat * gamma + beta

    @staticmethod
    def backward(ctx, dy):
        xhat, gamma, istd = ctx.saved_tensors
        dz = gamma * istd * (dy - dy.mean(0) - xhat * (dy * xhat).mean(0))
        return dz, (dy * xhat).sum(0), dy.sum(0), None, None


@contextlib.contextmanager
def batch_rule_backward():
    """Inside: the oracle's SineLayer computes frozen BatchNorm with the batch-statistics backward (float64 emulation of the mismatch)."""
    keep = orc.sine_layer

    def sine_layer(sd, name, x, train_bn=False, bn_out=None, mm=None):
        if name + ".norm.weight" not in sd:
            return keep(sd, name, x, train_bn, bn_out, mm)
        assert not train_bn
        z = orc.OMEGA0 * orc._linear(x, sd[name + ".linear.weight"], sd[name + ".linear.bias"], mm)
        return torch.sin(_BatchRuleOnRunningStats.apply(z, sd[name + ".norm.weight"], sd[name + ".norm.bias"], sd[name + ".norm.running_mean"],
                                                        sd[name + ".norm.running_var"]))

    orc.sine_layer = sine_layer
    try:
        yield
    finally:
        orc.sine_layer = keep
