"""The training engine's backward after a forward with frozen BatchNorm (train_bn = 0: running statistics, nothing updated) against the oracle's
float64 autograd of the same function (tests/frozen_bn_cases.py: cases, weights, inputs, references, the error measure).

The backward of a SineLayer with BatchNorm depends on the mode of its forward: with batch statistics dz = gamma istd (dy - mean(dy) - xhat mean(dy xhat)),
with running statistics dz = gamma istd dy.  A module in .eval() reaches the engine with gradients enabled through All_in_One_Eval.eval / get_loss at
every width without a fused kernel (fine-tuning with frozen BatchNorm, a gradient taken at validation time) and through the train_fwd_* ops at any.

A. image pass at the op level (training._image_pass, train_bn=False): W = 64 / 256 at 192 points (fp32 route: colreduce mode 1, then bn_bwd2 on its
   own) and at 1221 (row GEMMs: activation on load from a table built of the running statistics, activation backward in the dgrad epilogue, the dZ
   sweep riding in the weight-gradient kernel); W = 512 at 1155 (gemm_areg's form); W = 64 with the classic solar model (the solar branch's dgrad
   does fc9's activation backward).  Loss: a seeded linear functional of Rendered_Col, Albedo_Color, Sky_Col and PE.
B. per-point pass (train_fwd_points), seeded gradients on all five differentiable outputs.
C. sun-ray pass (train_fwd_solar): its backward meets no BatchNorm layer - the control.
D. the Python seam: T_NeRF(128, 4) / T_NeRF(100, 4) in .eval(), All_in_One_Eval.get_loss with gradients enabled, .backward() on the total.
E. no state leaks between the modes on one engine, in either order.   F. a frozen pass and its backward leave the module's state alone.

Every case: forward values at the tolerances of tests/test_gpu_parity.py::test_generic_width_runs_on_layerwise_engine (FWD_TOL), then every parameter
whose float64 gradient is non-zero - the biases in front of BatchNorm among them - at test_ragged_batch_vs_oracle's measure and bar (2e-3); every
other gradient None or exactly zero.  E_ref: the oracle in fp32 on the same measure (what fp32 arithmetic costs on these inputs).

Measured on an MI355X (worst gradient error; `before`: with the backward that did not know the mode of its forward):
    case                        E_ref      engine     before     worst tensor (engine; before)
    image_W64_12x16             4.1e-05    4.0e-05    3.8e+07    fc2.linear.bias; fc2.linear.bias
    image_W64_33x37             6.0e-05    1.2e-04    5.7e+05    fc2.norm.weight; fc2.linear.bias
    image_W256_12x16            3.9e-05    3.9e-05    3.5e+03    fc2.norm.weight; fc2.linear.bias
    image_W256_33x37            5.2e-05    8.8e-05    2.1e+03    fc2.norm.weight; fc2.linear.bias
    image_W512_35x33            4.8e-05    5.8e-05    8.0e+01    fc2.norm.weight; fc3.linear.bias
    image_W64_33x37_classic     3.9e-05    7.6e-05    8.5e+06    fc2.norm.weight; fc2.linear.bias
    points_W64_1221             5.1e-05    6.8e-05    4.3e+06    fc1.linear.bias; fc2.linear.bias
    solar_W64_12x16             3.4e-05    3.4e-05    3.4e-05    fc_solar_1.linear.weight (the control: the same before)
    solar_W64_33x37             6.3e-05    7.5e-05    7.5e-05    fc_solar_4.weight
    seam_W128_35x33             4.8e-05    2.8e-04    1.6e+05    fc_solar_4.bias; fc2.linear.bias
    seam_W100_35x33             5.3e-05    6.7e-05    3.3e+06    fc2.linear.weight; fc2.linear.bias
Forward values: at most 0.12 of their tolerance in the image, per-point and seam cases, 0.55 (PE) in the sun-ray cases.  The leak test: frozen then train
2.3e-04 / 3.9e-05 from a fresh train-mode step with a run-to-run spread of 3.3e-04 / 3.5e-05 (192 / 1221 points; the spread at 192 points is that of the biases in
front of BatchNorm, whose batch-mode gradient is rounding noise), train then frozen 1.8e-07 / 1.7e-07 with a spread of 1.4e-07 / 2.0e-07.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import frozen_bn_cases as fc
from frozen_bn_cases import BAR, BY_ID, CASES

pytestmark = pytest.mark.gpu

# (rtol, atol) against float64, as test_generic_width_runs_on_layerwise_engine holds the engine in eval mode (Rendered_Col: that file's parity bar)
FWD_TOL = {"Rho": (2e-4, 2e-5), "Col": (2e-4, 2e-5), "Solar_Vis": (2e-4, 2e-5), "Sky_Col": (2e-4, 2e-5), "Classes": (2e-4, 2e-5), "PS": (1e-4, 2e-5),
           "PE": (1e-4, 2e-5), "PV_Exact": (1e-4, 2e-5), "Rendered_Col": (1e-4, 2e-6), "Albedo_Color": (1e-4, 2e-6)}
DEAD = ("adjust_rho", "adjust_solar_vis", "adjust_sky_col")
IMAGE_OUT = ["Rendered_Col", "Albedo_Color", "Sky_Col", "PE", "Rendered_Col_Merged", "Albedo_Merged", "PV", "PS", "deltas", "Classes", "Rho", "Solar_Vis",
             "Col", "sample_pts", "Adjust"]


def _net(case, sd=None, train=False):
    import season_nerf_amd as sn
    net = sn.T_NeRF(case.W, case.C)
    net.load_state_dict(fc.weights(case) if sd is None else sd)
    return net.to("cuda").train(train)


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def _grads(net):
    return {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in net.named_parameters()}


def _image_step(net, case, inp, train_bn):
    """forward (train_fwd_image + compositing) and backward of the case's linear functional -> outputs, gradients"""
    import season_nerf_amd as sn
    from season_nerf_amd import training
    d = _cuda(inp["data"])
    eng = training._engine_for(net, case.R, case.R, case.S)
    eng.classic_solar = bool(case.classic)
    tv = sn.sample_parameters(case.S, eval_mode=True).cuda()
    res = training._image_pass(eng, d["Top"], d["Bot"], tv, d["Sun_Angle"], d["Time_Encoded"], train_bn, None, 1.0)
    training._after_train_forward(net)
    out = dict(zip(IMAGE_OUT, res))
    loss = sum((out[k] * w.cuda()).sum() for k, w in inp["w"].items())
    loss.backward()
    return out, _grads(net)


def _points_step(net, case, inp):
    from season_nerf_amd import training
    d = _cuda(inp["data"])
    eng = training._engine_for(net, case.R, case.R, 1)
    r = training._train_ops(eng).train_fwd_points(eng.handle, inp["X"].cuda(), d["Sun_Angle"], d["Time_Encoded"], False, net.n_classes, eng.param_list)
    out = dict(zip(["Rho", "Col", "Solar_Vis", "Sky_Col", "Classes"], r[:5]))
    loss = sum((out[k] * w.cuda()).sum() for k, w in inp["w"].items())
    loss.backward()
    return out, _grads(net)


def _solar_step(net, case, inp):
    import season_nerf_amd as sn
    from season_nerf_amd import training
    s = _cuda(inp["solar"])
    eng = training._engine_for(net, case.R, case.R, case.S)
    tv = sn.sample_parameters(case.S, eval_mode=True, include_end_pt=True).cuda()
    r = training._train_ops(eng, params_need_grad=False, kind="solar").train_fwd_solar(eng.handle, s["Top"], s["Bot"], tv, s["Sun_Angle"], False, eng.param_list)
    out = dict(zip(["Solar_Vis", "PV_Exact", "PE", "sky_raw", "Rho"], r[:5]))
    loss = sum((out[k] * w.cuda()).sum() for k, w in inp["w"].items())
    loss.backward()
    return out, _grads(net)


def _evaluator(case, inp):
    import season_nerf_amd as sn
    args = SimpleNamespace(n_samples=case.S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=True, Use_Solar=True, sc_lambda=fc.SC_LAMBDA,
                           number_low_frequency_cases=case.C)
    ev = sn.All_in_One_Eval(args, torch.device("cuda"), 10, False, None, np.eye(4), np.zeros(3))
    s = inp["solar"]
    ev.solar_creation_tool = lambda n, include_times=True: (s["Top"], s["Bot"], s["Sun_Angle"], torch.zeros(case.R, 4), None)
    return ev


def _seam_step(net, case, inp, ref):
    """a module in .eval() under the evaluator: eval() for the per-sample values, get_loss with gradients enabled, backward on the total"""
    ev = _evaluator(case, inp)
    assert not net.training and not net.fused
    with torch.no_grad():
        out = dict(ev.eval(inp["data"], net, 0, False))
    out["Sky_Col"] = out["Sky_Col"][:, 0, :]
    loss = ev.get_loss(inp["data"], net, 0, False)
    total = sum(v * w for v, w in loss.values())
    total.backward()
    for k in ("Solar_Correction", "Solar_Correction_2", "Sky_Color_Var", "Albedo_Color", "Color"):
        v = float(ref["out"]["loss_" + k])
        got = float(loss[k][0].detach())
        print(f"  loss {k:20s} {got:.7f} (float64 {v:.7f})")
        assert abs(got - v) <= 2e-5 * max(1.0, abs(v)) + 1e-6, k
    return out, _grads(net)


def _check_forward(case, out, ref):
    for k, (rtol, atol) in FWD_TOL.items():
        if k not in out or k not in ref["out"] or not torch.is_tensor(out[k]):
            continue
        a, b = out[k].detach().cpu().double(), ref["out"][k]
        if k == "Classes" and a.dim() == 2 and b.dim() == 3:
            b = b[:, 0, :]                                                  # one class vector per ray, as the op returns it
        a = a.reshape(b.shape)
        dev = float(((a - b).abs() / (atol + rtol * b.abs())).max())
        print(f"  {k:14s} max abs {float((a - b).abs().max()):.2e}, {dev:.2f} of the tolerance")
        np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=rtol, atol=atol, err_msg=f"{case.id} {k}")


def _check_grads(case, grads, ref):
    names, gmax = fc.live(ref)
    e32 = fc.worst(fc.grad_errors(fc.run_oracle(case, torch.float32)["grads"], ref))
    err = fc.grad_errors(grads, ref)
    w, k = fc.worst(err)
    print(f"  {case.id}: {len(names)} tensors compared, gmax {gmax:.3e};  E_ref {e32[0]:.2e} ({e32[1]});  engine worst {w:.2e} ({k})")
    for n in sorted(err, key=err.get, reverse=True)[:4]:
        print(f"      {n:40s} {err[n]:.2e}")
    for n, g in grads.items():
        if n not in names:          # no path in float64 (the dead heads; whatever the pass does not differentiate): nothing may arrive
            assert g is None or float(g.abs().max()) == 0.0, (case.id, n)
    assert all(n in grads for n in names) and not any(n.split(".")[0] in DEAD for n in names)
    assert w < BAR, (case.id, w, k)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_frozen_batchnorm_backward_vs_float64(case):
    ref, inp = fc.reference(case), fc.inputs(case)
    net = _net(case)
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    if case.kind == "image":
        out, grads = _image_step(net, case, inp, False)
    elif case.kind == "points":
        out, grads = _points_step(net, case, inp)
    elif case.kind == "solar":
        out, grads = _solar_step(net, case, inp)
    else:
        out, grads = _seam_step(net, case, inp, ref)
    _check_forward(case, out, ref)
    _check_grads(case, grads, ref)
    for k, v in net.state_dict().items():          # neither the parameters nor the running statistics moved
        assert torch.equal(v, before[k]), k


def _spread(a, b, ref):
    """largest difference of two gradient sets on the measure of the gradient test (scales from `ref`)"""
    gmax = max(float(v.abs().max()) for v in ref.values() if v is not None)
    worst = 0.0
    for k, r in ref.items():
        if r is None:
            assert a[k] is None and b[k] is None, k
            continue
        worst = max(worst, float((a[k] - b[k]).abs().max()) / max(float(r.abs().max()), 1e-3 * gmax))
    return worst


@pytest.mark.parametrize("cid", ["image_W64_12x16", "image_W64_33x37"])
def test_no_state_leaks_between_modes(cid):
    """One engine: a frozen forward + backward, then a .train() forward + backward on the same inputs - the second gradients are those of a fresh module
    that only ran the train-mode step, within twice the run-to-run spread of two fresh modules (the atomic reductions).  Then the other order; there the
    fresh modules start from the state the train-mode step left (it moved the running statistics the frozen step reads)."""
    case = BY_ID[cid]
    inp = fc.inputs(case)

    def step(net, train):
        net.train(train)
        net.zero_grad(set_to_none=True)
        return _image_step(net, case, inp, train)[1]

    f1, f2 = step(_net(case), True), step(_net(case), True)
    noise = _spread(f1, f2, f1)
    net = _net(case)
    frozen_first = step(net, False)
    leak = _spread(step(net, True), f1, f1)
    print(f"  {cid}: frozen then train: {leak:.2e} from a fresh train-mode step (run-to-run {noise:.2e})")
    assert leak <= 2 * noise, (leak, noise)
    assert _spread(frozen_first, f1, f1) > 100 * BAR          # the two modes' gradients are far apart: a leak would show

    net = _net(case)
    step(net, True)
    sd = {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}
    g1, g2 = step(_net(case, sd), False), step(_net(case, sd), False)
    noise = _spread(g1, g2, g1)
    leak = _spread(step(net, False), g1, g1)
    print(f"  {cid}: train then frozen: {leak:.2e} from a fresh frozen step (run-to-run {noise:.2e})")
    assert leak <= 2 * noise, (leak, noise)


def test_frozen_pass_has_no_side_effects():
    """A train_bn = 0 pass and its backward on a module in .eval(): running_mean / running_var bit-identical, num_batches_tracked unchanged, the packed
    inference weights still valid (same packed object, same handle, the same fused render bit for bit)."""
    from season_nerf_amd import training
    case = BY_ID["image_W64_33x37"]
    inp = fc.inputs(case)
    net = _net(case)
    net.precision = "bf16x3"
    ev = _evaluator(case, inp)
    with torch.no_grad():
        training.eval_train(ev, inp["data"], net, False)          # the engine exists (its parameter store has adopted the module's tensors)
        rgb0 = ev.eval(inp["data"], net, 0, False)["Rendered_Col"].clone()      # .eval() at a fused width: the packed model
    assert net.fused
    packed, handle, sig = net.op_model(), net.device_model(), net.__dict__["_packed_sig"]
    assert sig is not None
    before = {k: v.detach().clone() for k, v in net.state_dict().items()}
    out = training.eval_train(ev, inp["data"], net, False)          # frozen BatchNorm, gradients enabled
    (out["Rendered_Col"].sum() + out["PE"].sum()).backward()
    torch.cuda.synchronize()
    assert float(dict(net.named_parameters())["G_NeRF_net.fc2.linear.bias"].grad.abs().max()) > 0
    after = net.state_dict()
    for k, v in before.items():
        assert torch.equal(after[k], v), k
    assert int(after["G_NeRF_net.fc2.norm.num_batches_tracked"]) == int(before["G_NeRF_net.fc2.norm.num_batches_tracked"]) == 0
    assert net.__dict__["_packed_sig"] == sig and net.op_model() is packed and net.device_model() == handle
    with torch.no_grad():
        rgb1 = ev.eval(inp["data"], net, 0, False)["Rendered_Col"]
    assert torch.equal(rgb0, rgb1)
