"""GPU tests of the shadow-walk feature: `season_nerf::shadow_walk` (csrc/mlp_device.h RayShadow; shadow_walk_kernel<64|256>, shadow_walk_ks_kernel<512>)
against the per-sample path (`forward_Solar` on the sample points, float64 sums), its persistent loop and tile tails, the reference's recorded per-sample
arrays and scores (tests/golden/shadow_points.npz), the fallback for networks the kernels do not serve, the mirrors of the reference's call boundary and
the op's schema, fake kernel and argument checks.

Tolerances.  Counts (slots 0-2): a sample whose learned visibility (the per-sample path's fp32 value) or float64 PV lies within 1e-6 of .5 may fall on
either side; a ray without such a sample must give equal integers, another may differ by at most their number.  Sums (slots 3-7): the measured rule of
test_gpu_compositing.py (`_check`), as test_gpu_surface.py::test_kernel_vs_float64 applies it: within 4 * (E_ref + 2^-24 * scale), E_ref = the deviation
of the same formulas in CPU fp32 from float64; scale = S for sum (PV - vis)^2 and sum |PV - vis| (S terms of at most 1: the rule on the sums divided by
S, at unit scale, as sum PS s is divided by S - 1 there), 1 for sum PS vis and sum PS, the ray's optical depth for the last.

Against the reference: the band, E_VIS and E_PV of tests/test_shadow_host.py, measured by `test_per_sample_deviation` below."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc
from test_gpu_compositing import SENT, _check, _report
from test_gpu_surface import close, net_of
from test_shadow_host import BAND, E_PV, E_VIS, KEYS, eight_sums, fixture, fixture_rays, in_band, reference_error
from test_surface_host import TAGS

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEAR = 1e-6
NAMES = ("tp", "n_exact", "n_est", "sq_err", "abs_err", "ps_vis", "acc", "carry")


def sun_rays(R, seed):
    """R rays through ground points towards R different suns, as eval_shadow_data lays them (ground -+ sun / sun_z).  The suns of the odd rays stand low
    (15 - 35 degrees): those rays leave the cube.  The sun vector handed to the network is not a unit vector (x 0.8 .. 1.2): nothing normalises it."""
    rng = np.random.Generator(np.random.PCG64(seed))
    el = np.where(np.arange(R) % 2 == 1, rng.uniform(15, 35, R), rng.uniform(60, 89, R)) * np.pi / 180
    az = rng.uniform(0, 2 * np.pi, R)
    v = np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], 1)
    g3 = np.concatenate([rng.uniform(-1, 1, (R, 2)), np.zeros((R, 1))], 1)
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV).contiguous()
    return f(g3 + v / v[:, 2:]), f(g3 - v / v[:, 2:]), f(v * rng.uniform(0.8, 1.2, (R, 1)))


def per_sample(net, top, bot, sun, S, zero_oob):
    """The per-sample path: `forward_Solar` on the sample points -> rho, vis, delta [R,S] (fp32, CPU) with delta zeroed outside the cube on request."""
    from season_nerf_amd.evaluator import sample_parameters_on
    R = top.shape[0]
    tv = sample_parameters_on(torch.device(DEV), S, eval_mode=True)
    t = tv.reshape(1, S, 1)
    pts = top.unsqueeze(1) * (1 - t) + bot.unsqueeze(1) * t
    delta = (torch.sqrt(((top - bot) ** 2).sum(1)) / S).reshape(-1, 1).expand(R, S)
    oob = (pts.abs() > 1).any(2)
    if zero_oob:
        delta = torch.where(oob, torch.zeros_like(delta), delta)
    with torch.no_grad():
        rho, vis, _ = net.forward_Solar(pts.reshape(-1, 3), sun.unsqueeze(1).expand(R, S, 3).reshape(-1, 3), torch.zeros(R * S, 4, device=DEV))
    return rho.detach().reshape(R, S).cpu(), vis.detach().reshape(R, S).cpu(), delta.cpu().contiguous(), oob.cpu()


def statement(rho, vis, delta):
    """The eight sums and PV in the dtype of the arguments; PV as get_PV forms it."""
    y = rho * delta
    c = torch.cumsum(torch.cat([torch.zeros_like(y[:, :1]), y], 1), 1)
    pv = torch.exp(-c[:, :-1])
    return eight_sums(pv, vis, y), pv


def check_eight(kernel, family, got, rho, vis, delta):
    """got [R,8] (fp32) against the float64 statement on the per-sample path's rho and vis, by the rules in the module docstring."""
    S = rho.shape[1]
    got = got.detach().cpu()
    ref64, pv64 = statement(rho.double(), vis.double(), delta.double())
    ref32, _ = statement(rho, vis, delta)
    near = (((vis.double() - .5).abs() <= NEAR) | ((pv64 - .5).abs() <= NEAR)).sum(1)
    for k in range(3):
        diff = (got[:, k].double() - ref64[:, k]).abs()
        assert bool((got[:, k] == got[:, k].round()).all()), f"{kernel}/{family}/{NAMES[k]}: not an integer"
        assert bool((diff <= near).all()), (f"{kernel}/{family}/{NAMES[k]}: counts differ by up to {float(diff.max())} on rays with "
                                            f"{near[diff > near].tolist()} samples within {NEAR} of .5")
    for k in (3, 4):
        _check(kernel, family, NAMES[k], got[:, k] / S, ref64[:, k] / S, ref32[:, k] / S, unit_scale=True)
    for k in (5, 6):
        _check(kernel, family, NAMES[k], got[:, k], ref64[:, k], ref32[:, k], unit_scale=True)
    _check(kernel, family, NAMES[7], got[:, 7], ref64[:, 7], ref32[:, 7])
    return int((near > 0).sum())


@pytest.mark.parametrize("R,S", [(1, 96), (3, 96), (5, 96), (37, 96), (37, 1), (37, 31), (37, 32), (37, 33), (37, 40)])
@pytest.mark.parametrize("W", [64, 256, 512])
def test_kernel_vs_per_sample_path(golden_dir, W, R, S):
    """The kernel against the parent's per-sample path; no reference involved."""
    import season_nerf_amd as sn
    net = net_of(golden_dir, f"sharp_W{W}")
    assert net.resolved_precision == "bf16x3"
    top, bot, sun = sun_rays(R, 1000 * W + 10 * R + S)
    for zero_oob in (False, True):
        rho, vis, delta, oob = per_sample(net, top, bot, sun, S, zero_oob)
        assert R < 4 or S < 4 or bool(oob.any())
        sw = sn.shadow_walk(net, top, bot, sun, S, zero_oob=zero_oob)
        assert sw.sums.shape == (R, 8) and sw.sums.dtype == torch.float32 and sw.n_samples == S
        n_near = check_eight("shadow_walk", f"W{W}", sw.sums, rho, vis, delta)
        rs = sn.ray_surface(net, top, bot, S, zero_oob=zero_oob, early_out=False)
        same = torch.equal(sw.acc, rs.acc) and torch.equal(sw.carry, rs.carry)
        print(f"  W={W} R={R} S={S} zero_oob={zero_oob}: rays with a sample within {NEAR} of .5: {n_near}; sum PS and optical depth "
              f"{'bit-identical to' if same else 'differ in bits from'} ray_surface's")
        np.testing.assert_allclose(sw.acc.cpu().numpy(), rs.acc.cpu().numpy(), rtol=1e-6, atol=0)
        np.testing.assert_allclose(sw.carry.cpu().numpy(), rs.carry.cpu().numpy(), rtol=1e-6, atol=0)
    _report("shadow_walk")


@pytest.mark.parametrize("W,rays_per_tile", [(64, 4), (512, 2)])
def test_persistent_loop_and_tile_tail(golden_dir, W, rays_per_tile):
    """More tiles than workgroups and a last tile with one ray: every row written, nothing around them, two launches bit for bit, and the rows of the
    first rays the same as in a launch of those rays alone."""
    import season_nerf_amd as sn
    from season_nerf_amd.evaluator import sample_parameters_on
    L = sn._lib.lib()
    net = net_of(golden_dir, f"sharp_W{W}")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    R, S, pad = rays_per_tile * (n_cu + 3) + 1, 33, 4
    top, bot, sun = sun_rays(R, W)
    tv = sample_parameters_on(torch.device(DEV), S, eval_mode=True)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(n):
        buf = torch.full(((n + 2 * pad) * 8,), SENT, device=DEV)
        assert buf.data_ptr() % 32 == 0
        rc = L.snerf_field_shadow_walk(C.c_void_p(net.device_model()), n, S, top.data_ptr(), bot.data_ptr(), sun.data_ptr(), tv.data_ptr(), 2,
                                       buf.data_ptr() + pad * 32, st)
        assert rc == 0, L.snerf_last_error()
        torch.cuda.synchronize()
        b = buf.cpu().reshape(n + 2 * pad, 8)
        assert bool((b[:pad] == SENT).all()) and bool((b[n + pad:] == SENT).all()), "a row outside the output was written"
        assert not bool((b[pad:n + pad] == SENT).any()), f"rows left unwritten: {torch.nonzero((b[pad:n + pad] == SENT).any(1)).reshape(-1).tolist()}"
        return b[pad:n + pad]

    a, b = launch(R), launch(R)
    assert torch.equal(a, b)
    assert bool(torch.isfinite(a).all())
    assert torch.equal(a[:37], launch(37))
    rho, vis, delta, _ = per_sample(net, top[-9:].contiguous(), bot[-9:].contiguous(), sun[-9:].contiguous(), S, True)
    check_eight("shadow_walk", f"W{W} tail", a[-9:], rho, vis, delta)


def _device_arrays(golden_dir, g, tag, Z):
    """eval_shadow_data on the fixture's configuration with the network of `tag`."""
    import season_nerf_amd as sn
    return sn.eval_shadow_data(net_of(golden_dir, tag), g["shadow_angles"], g["ground_points"], Z, g["world_center_LLA"], g["W2L_H"], 15000, DEV)


def test_per_sample_deviation(golden_dir):
    """The measurement behind E_VIS, E_PV and the band of test_shadow_host.py: the per-sample path (`eval_shadow_data`: forward_Solar + get_PV, code the
    shadow walk does not run) against the reference's arrays, over the whole fixture.

    And `eval_shadow_data` against the fixture.  The sharp sets scale the density head by 64 and the low suns make the steps long, so the reference's
    own fp32 arrays stand up to 7e-5 from float64 here: the band is the measured rule of test_gpu_compositing.py on the reference's own error, per set
    4 * (E_ref + 2^-24), E_ref = max |reference fp32 - CPU oracle in float64| (test_shadow_host.reference_error); the raw sky colour at the parity
    tests' band for raw head outputs (rtol 1e-4, atol 1e-4)."""
    g = fixture(golden_dir)
    e_vis = e_pv = 0.0
    for tag in TAGS:
        for Z in (int(z) for z in g["Z_list"]):
            ex, es, sky = _device_arrays(golden_dir, g, tag, Z)
            M, G = g["shadow_angles"].shape[0], g["ground_points"].shape[0]
            assert ex.shape == (M, G, Z, 1) and es.shape == (M, G, Z, 1) and sky.shape == (M, 3) and ex.dtype == np.float64
            dv, dp = np.abs(es[..., 0] - g[f"{tag}_Z{Z}_Est_Vis"]).max(), np.abs(ex[..., 0] - g[f"{tag}_Z{Z}_Exact_Vis"]).max()
            r_pv, r_vis = reference_error(golden_dir, g, tag, Z)
            print(f"  {tag} Z={Z}: max |vis - Est_Vis_ref| {dv:.4e} (reference's own error {r_vis:.2e})   max |PV - Exact_Vis_ref| {dp:.4e} ({r_pv:.2e})")
            e_vis, e_pv = max(e_vis, dv), max(e_pv, dp)
            assert dv <= 4 * (r_vis + 2.0 ** -24), (tag, Z, "Est_Vis", dv, r_vis)
            assert dp <= 4 * (r_pv + 2.0 ** -24), (tag, Z, "Exact_Vis", dp, r_pv)
            close(f"{tag} Z={Z} Sky_Col", sky, g[f"{tag}_Z{Z}_Sky_Col"], rtol=1e-4, atol=1e-4)
    print(f"  E_VIS = {e_vis:.4e}   E_PV = {e_pv:.4e}   band = 2 max = {2 * max(e_vis, e_pv):.4e}   (recorded: {E_VIS:.4e}, {E_PV:.4e}, {BAND:.4e})")
    assert e_vis <= E_VIS and e_pv <= E_PV, "the recorded maxima no longer bound the per-sample path's deviation"


@pytest.mark.parametrize("Z", [96, 40])
@pytest.mark.parametrize("tag", TAGS)
def test_walk_vs_reference(golden_dir, tag, Z):
    """Test_Shadow_Points(full_return=False)'s rays through the kernel against the reference's per-sample arrays: per ray each count within the number
    of that ray's reference samples inside the band; Loss and Avg_Error within what E_VIS + E_PV allows: |d_dev - d_ref| <= E per sample, so the mean
    absolute error moves by at most E and the mean squared one by at most 2 E Avg_Error_ref + E^2."""
    import season_nerf_amd as sn
    g = fixture(golden_dir)
    net = net_of(golden_dir, tag)
    assert net.resolved_precision == "bf16x3"
    exact, est, ref = g[f"{tag}_Z{Z}_Exact_Vis"], g[f"{tag}_Z{Z}_Est_Vis"], dict(zip(KEYS, g[f"{tag}_Z{Z}_scores"]))
    M, G = exact.shape[:2]
    top, bot, sun = (a.to(DEV) for a in fixture_rays(g))
    sw = sn.shadow_walk(net, top, bot, sun, Z)
    got = sw.sums.cpu().double().reshape(M, G, 8)
    ex64, es64 = exact.astype(np.float64), est.astype(np.float64)
    allowed = in_band(exact, est, BAND).sum(2)
    counts = {"tp": ((ex64 > .5) & (es64 > .5)).sum(2), "n_exact": (ex64 > .5).sum(2), "n_est": (es64 > .5).sum(2)}
    for k, name in enumerate(("tp", "n_exact", "n_est")):
        diff = np.abs(got[..., k].numpy() - counts[name])
        print(f"  {tag} Z={Z} {name}: rays that differ {int((diff > 0).sum())} of {M * G}, largest difference {int(diff.max())}; rays with a sample in the band {int((allowed > 0).sum())}")
        assert (diff <= allowed).all(), (name, np.argwhere(diff > allowed).tolist())
    sc = sw.scores()
    for k in KEYS:
        print(f"  {tag} Z={Z} {k:14s} {sc[k]:.9f} (reference {ref[k]:.9f})")
    E = E_VIS + E_PV
    assert abs(sc["Avg_Error"] - ref["Avg_Error"]) <= E, (sc["Avg_Error"], ref["Avg_Error"], E)
    assert abs(sc["Loss"] - ref["Loss"]) <= 2 * E * ref["Avg_Error"] + E * E, (sc["Loss"], ref["Loss"], E)


def test_mirror_short_return(golden_dir):
    """Test_Shadow_Points(full_return=False) lays the rays itself and goes through shadow_walk: the same scores as the rays of the fixture by hand;
    an empty set of suns gives NaN scores."""
    import season_nerf_amd as sn
    g = fixture(golden_dir)
    net = net_of(golden_dir, "sharp_W64")
    ang = g["shadow_angles"]
    r = sn.Test_Shadow_Points(net, ang[:2], ang[2:], ang[:0], ang, g["ground_points"], g["world_center_LLA"], g["W2L_H"], DEV, Z_points=40, full_return=False)
    assert list(r) == ["Training", "Testing", "Near", "Full"] and all(list(v) == list(KEYS) for v in r.values())
    top, bot, sun = (a.to(DEV) for a in fixture_rays(g))
    sw = sn.shadow_walk(net, top, bot, sun, 40)
    G = g["ground_points"].shape[0]
    mask = torch.zeros(ang.shape[0], G, dtype=torch.bool)
    mask[:2] = True
    for k in KEYS:
        assert r["Full"][k] == sw.scores()[k] and r["Training"][k] == sw.scores(mask)[k] and r["Testing"][k] == sw.scores(~mask)[k], k
        assert np.isnan(r["Near"][k])
    full = sn.Test_Shadow_Points(net, ang[:1], ang[1:2], ang[:0], ang[2:3], g["ground_points"][:5], g["world_center_LLA"], g["W2L_H"], DEV, Z_points=40)
    assert full["Training_Results"]["Exact_Vis"].shape == (1, 5, 40, 1) and full["Near_Results"]["Est_Vis"].shape == (0, 5, 40, 1)
    an = sn.shadow_anaylysis(full["Ground_Points"], full["Sun_El_Az"]["Full_Walk"], full["Full_Results"])
    assert list(an) == list(KEYS)


@pytest.mark.parametrize("kind", ["i8x3", "W128", "train_mode"])
def test_fallback(golden_dir, kind):
    """Networks the kernels do not serve get the same eight numbers from `forward_Solar` on the sample points: int8 digits, a width without a fused
    kernel, and a module in training mode (batch statistics over the chunk the fallback forms: all R x S points at once)."""
    import season_nerf_amd as sn
    from season_nerf_amd import render as R_
    if kind == "W128":
        net = sn.T_NeRF(128, 4)
        net.load_state_dict(orc.init_weights(128, 4, 2))
        net = net.to(DEV).eval()
        assert not net.fused
    elif kind == "i8x3":
        net = net_of(golden_dir, "init_W64_s2", "i8x3")
        assert net.resolved_precision == "i8x3"
    else:
        net = sn.T_NeRF(64, 4)
        net.load_state_dict(orc.init_weights(64, 4, 2))
        net.precision = "bf16x3"
        net = net.to(DEV).train()
    assert not (R_._walks(net) and not net.training)
    R, S = 37, 33
    top, bot, sun = sun_rays(R, 5)
    for zero_oob in (False, True):
        rho, vis, delta, _ = per_sample(net, top, bot, sun, S, zero_oob)
        sw = sn.shadow_walk(net, top, bot, sun, S, zero_oob=zero_oob)
        assert sw.sums.shape == (R, 8)
        check_eight("shadow_walk fallback", kind, sw.sums, rho, vis, delta)


def test_op(golden_dir):
    """opcheck (schema and fake kernel), argument errors, a NULL model, and two launches bit for bit."""
    import season_nerf_amd as sn
    from season_nerf_amd.evaluator import sample_parameters_on
    ops = sn.ops.load()
    net = net_of(golden_dir, "sharp_W64")
    h = net.device_model()
    top, bot, sun = sun_rays(37, 1)
    tv = sample_parameters_on(torch.device(DEV), 40, eval_mode=True)
    a = ops.shadow_walk(h, top, bot, sun, tv, 2)
    b = ops.shadow_walk(h, top, bot, sun, tv, 2)
    assert a.shape == (37, 8) and a.dtype == torch.float32 and a.device == top.device and torch.equal(a, b)
    assert ops.shadow_walk(h, top[:0], bot[:0], sun[:0], tv, 0).shape == (0, 8)
    torch.library.opcheck(torch.ops.season_nerf.shadow_walk.default, (h, top, bot, sun, tv, 2), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError, match="top"):
        ops.shadow_walk(h, top[:, :2].contiguous(), bot, sun, tv, 0)
    with pytest.raises(RuntimeError, match="bot"):
        ops.shadow_walk(h, top, bot[:5], sun, tv, 0)
    with pytest.raises(RuntimeError, match="sun"):
        ops.shadow_walk(h, top, bot, sun[:5], tv, 0)
    with pytest.raises(RuntimeError, match="float32"):
        ops.shadow_walk(h, top.double(), bot, sun, tv, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.shadow_walk(h, top, bot, sun.cpu(), tv, 0)
    with pytest.raises(RuntimeError, match="tvals"):
        ops.shadow_walk(h, top, bot, sun, tv.reshape(1, -1), 0)
    with pytest.raises(RuntimeError, match="flags"):
        ops.shadow_walk(h, top, bot, sun, tv, 4)
    with pytest.raises(RuntimeError, match="NULL"):
        ops.shadow_walk(0, top, bot, sun, tv, 0)
    net8 = net_of(golden_dir, "init_W64_s2", "i8x3")
    with pytest.raises(RuntimeError, match="snerf_field_shadow_walk"):
        ops.shadow_walk(net8.device_model(), top, bot, sun, tv, 0)
    with pytest.raises(ValueError, match="shadow_walk"):
        sn.shadow_walk(net, top, bot, sun[:5], 40)
