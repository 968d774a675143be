"""The references of tests/frozen_bn_cases.py on the CPU: the oracle's frozen SineLayer against torch.nn.BatchNorm1d.eval() autograd, and the two
conditions that keep the case list honest - the batch-statistics backward rule applied to running statistics (what the engine computed before its
backward knew the mode) must miss the frozen reference by far more than the GPU test's bar, and the oracle in fp32 must sit far below it."""
import pytest
import torch

import frozen_bn_cases as fc
from frozen_bn_cases import CASES, BAR
from oracle import season_nerf_oracle as orc


def test_frozen_sine_layer_is_batchnorm1d_eval():
    """sin(BN_eval(30 (x W^T + b))) of the oracle in float64 against torch.nn.Linear + torch.nn.BatchNorm1d(...).eval(): value and every gradient
    (weight, bias, gamma, beta, input) to 1e-12 of the tensor's largest entry."""
    case = fc.BY_ID["image_W64_33x37"]
    sd = orc.cast_weights(fc.weights(case), torch.float64)
    name, W, N = "G_NeRF_net.fc3", case.W, 301
    g = torch.Generator().manual_seed(5)
    x0 = torch.rand(N, W, generator=g, dtype=torch.float64) * 2 - 1
    dy = torch.randn(N, W, generator=g, dtype=torch.float64)
    keys = [".linear.weight", ".linear.bias", ".norm.weight", ".norm.bias"]

    p = {k: (v.clone().requires_grad_(True) if any(k == name + s for s in keys) else v) for k, v in sd.items()}
    x = x0.clone().requires_grad_(True)
    y = orc.sine_layer(p, name, x, train_bn=False)
    (y * dy).sum().backward()
    got = [y.detach(), x.grad] + [p[name + s].grad for s in keys]

    lin = torch.nn.Linear(W, W).double()
    bn = torch.nn.BatchNorm1d(W, eps=orc.BN_EPS).double()
    with torch.no_grad():
        lin.weight.copy_(sd[name + ".linear.weight"]); lin.bias.copy_(sd[name + ".linear.bias"])
        bn.weight.copy_(sd[name + ".norm.weight"]); bn.bias.copy_(sd[name + ".norm.bias"])
        bn.running_mean.copy_(sd[name + ".norm.running_mean"]); bn.running_var.copy_(sd[name + ".norm.running_var"])
    bn.eval()
    x2 = x0.clone().requires_grad_(True)
    y2 = torch.sin(bn(orc.OMEGA0 * lin(x2)))
    (y2 * dy).sum().backward()
    want = [y2.detach(), x2.grad, lin.weight.grad, lin.bias.grad, bn.weight.grad, bn.bias.grad]
    assert torch.equal(bn.running_mean, sd[name + ".norm.running_mean"]) and int(bn.num_batches_tracked) == 0
    for label, a, b in zip(["y", "dx"] + keys, got, want):
        err = float((a - b).abs().max()) / float(b.abs().max())
        print(f"  {label:16s} {err:.2e}")
        assert err <= 1e-12, (label, err)
    assert float(lin.bias.grad.abs().max()) > 1e-3 * float(lin.weight.grad.abs().max())      # the bias in front of frozen BatchNorm has a gradient


def _trunk(names):
    return [k for k in names if k.startswith("G_NeRF_net.fc") and k.split(".")[1] in {f"fc{i}" for i in range(1, 10)}]


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_case_separates_the_two_backward_rules(case):
    """Every case whose backward meets a BatchNorm layer: a float64 emulation of the batch-statistics rule on running statistics misses the frozen
    reference by more than 100 x BAR on at least one trunk tensor, so a test at BAR tells the two apart whatever weights or sizes the list holds later.
    The sun-ray cases are the control: their backward ends above the trunk, and the emulation must equal the reference there."""
    ref = fc.reference(case)
    with fc.batch_rule_backward():
        emu = fc.run_oracle(case, torch.float64)
    assert abs(emu["loss"] - ref["loss"]) <= 1e-13 * abs(ref["loss"])       # the same forward
    err = fc.grad_errors(emu["grads"], ref)
    trunk = {k: err[k] for k in _trunk(err)}
    if case.kind == "solar":
        assert not trunk and max(err.values()) == 0.0, fc.worst(err)
        return
    w, k = fc.worst(trunk)
    print(f"  {case.id}: batch rule on running statistics is off by {w:.2e} ({k}) = {w / BAR:.1e} x the bar")
    assert w > 100 * BAR, (w, k)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_fp32_oracle_is_far_below_the_bar(case):
    """The same formulas in fp32 stay below a tenth of BAR against float64: the condition under which a correct fp32 implementation can meet BAR.
    Also what every case must have: the dead heads without a gradient, and every other parameter of the differentiated branches live."""
    ref = fc.reference(case)
    got = fc.run_oracle(case, torch.float32)
    w, k = fc.worst(fc.grad_errors(got["grads"], ref))
    print(f"  {case.id}: E_ref {w:.2e} ({k})")
    assert w < BAR / 10, (w, k)
    names, _ = fc.live(ref)
    for k, g in ref["grads"].items():
        if k.split(".")[0] in ("adjust_rho", "adjust_solar_vis", "adjust_sky_col"):
            assert g is None or float(g.abs().max()) == 0.0, k
    if case.kind != "solar":
        for i in range(2, 10):                                              # frozen mode: the biases in front of BatchNorm carry a real gradient
            assert f"G_NeRF_net.fc{i}.linear.bias" in names and f"G_NeRF_net.fc{i}.norm.weight" in names
