"""GPU tests of the solar audit: `snerf_field_solar_audit` / `season_nerf::solar_audit` (csrc/mlp_device.h RayAudit; solar_audit_kernel<64|256>,
solar_audit_ks_kernel<512>) against the path the feature does not touch (`season_nerf::ray_visibility` on secondary rays formed on the host side by
`_exact_solar_visibility`'s float64 formula), its sums against float64 sums of its own per-sample output, the persistent loop, the Python boundary
(`solar_audit`, `audit_by_dir`, `eval_solar_data`, the fallback) against the reference's recorded arrays (tests/golden/solar_audit.npz) and the op.

Exact_Solar, bit for bit.  `ray_visibility` has its early-out always on (its A/B switch is read from the environment once per process), and it skips the
remaining passes of a group of rays only after every ray of the group has passed optical depth 18.  So:
  * a ray whose `ray_visibility` is >= exp(-18) was walked in full there: the audit kernel without early-out (flags bit2) must give the same bits; on the
    other rays both values must lie below exp(-18) (at S <= 32 there is one pass and nothing to skip: every ray is compared bit for bit);
  * with the early-out on in both, the groups of the two kernels coincide when S % 4 == 0 (W = 64 / 256: four consecutive rays) or S % 2 == 0 (W = 512: two):
    every ray must then give the same bits; otherwise the values lie within 2 exp(-18) of the kernel's own no-early-out values.
Sums: slots 0-2 equal the counts of the kernel's own `d_exact` against V; slots 3-7 lie within 2 (S + 2) 2^-24 sum |terms| of the float64 sums of the
same fp32 terms (fp32 summation of S terms, one rounding per product)."""
import ctypes as C

import numpy as np
import pytest
import torch

from test_audit_host import ARRAYS, BAND, BAND_SURF, E_EST, E_EXACT, E_SURF, S_LIST, SUN_EL_AZ, VIEWS, fixture, key_of, ps_of, reference_of
from test_gpu_compositing import SENT
from test_gpu_surface import net_of
from test_surface_host import TAGS

pytestmark = pytest.mark.gpu
DEV = "cuda"
PAD = 4
SAT = float(np.exp(np.float32(-18.0)))
S_ALL = [1, 2, 3, 5, 31, 32, 33, 38, 40, 96]
SUNS = np.array([[0.55, -0.35, 0.45], [-0.2, 0.3, 0.9]], dtype=np.float64)      # a low sun (secondary rays leave through the sides) and a high one


def view_rays(R, seed):
    """R primary rays of a view: parallel columns through random ground points, tilted 0 - 25 degrees off nadir, top at z = +1, bot at z = -1."""
    rng = np.random.Generator(np.random.PCG64(seed))
    el, az = np.deg2rad(rng.uniform(65, 90)), rng.uniform(0, 2 * np.pi)
    v = np.array([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)])
    g3 = np.concatenate([rng.uniform(-0.9, 0.9, (R, 2)), np.zeros((R, 1))], 1)
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV).contiguous()
    return f(g3 + v / v[2]), f(g3 - v / v[2])


def v_and_ps(R, S, seed):
    """V and PS [R S + 8] in [0,1], every seventh V at exactly .5, the eight values past R S NaN (they must reach no output)."""
    g = torch.Generator().manual_seed(seed)
    V, PS = torch.rand(R * S + 8, generator=g), torch.rand(R * S + 8, generator=g)
    V[::7] = 0.5
    V[R * S:], PS[R * S:] = float("nan"), float("nan")
    return V.to(DEV), PS.to(DEV)


def audit_call(net, top, bot, tv, sun, V, PS, flags, n=None):
    """The C call with sentinel rows in front of and behind d_out and d_exact -> out [n,8], exact [n,S] (CPU)."""
    import season_nerf_amd as sn
    L = sn._lib.lib()
    n, S = top.shape[0] if n is None else n, tv.numel()
    out = torch.full(((n + 2 * PAD) * 8,), SENT, device=DEV)
    ex = torch.full(((n + 2 * PAD) * S,), SENT, device=DEV)
    assert out.data_ptr() % 32 == 0
    sun3 = (C.c_double * 3)(*[float(x) for x in sun])
    rc = L.snerf_field_solar_audit(C.c_void_p(net.device_model()), n, S, top.data_ptr(), bot.data_ptr(), tv.data_ptr(), C.addressof(sun3), V.data_ptr(),
                                   PS.data_ptr(), flags, out.data_ptr() + PAD * 32, ex.data_ptr() + PAD * S * 4, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.snerf_last_error()
    torch.cuda.synchronize()
    o, x = out.cpu().reshape(n + 2 * PAD, 8), ex.cpu().reshape(n + 2 * PAD, S)
    for name, b in (("d_out", o), ("d_exact", x)):
        assert bool((b[:PAD] == SENT).all()) and bool((b[n + PAD:] == SENT).all()), f"{name}: a row outside the output was written"
        assert not bool((b[PAD:n + PAD] == SENT).any()), f"{name}: values left unwritten"
        assert bool(torch.isfinite(b).all()), f"{name}: not finite"
    return o[PAD:n + PAD].clone(), x[PAD:n + PAD].clone()


def secondary_rays(top, bot, tv, sun):
    """Tops and bottoms of the secondary rays of every sample, [R S, 3]: the points as the kernels form them, then `_exact_solar_visibility`'s formula."""
    t = tv.reshape(1, -1, 1)
    b_ = (top.unsqueeze(1) * (1.0 - t) + bot.unsqueeze(1) * t).reshape(-1, 3).contiguous()
    sun_d = torch.tensor(sun, dtype=torch.float32, device=DEV)
    s64 = torch.tensor(sun, dtype=torch.float64, device=DEV).reshape(1, 3)
    K = (1.0 - b_[:, 2]) / sun_d[2]
    return (b_.double() + K.double().unsqueeze(1) * s64).float().contiguous(), b_


def ray_visibility(net, top, bot, tv, sun):
    from season_nerf_amd.network import _ops
    t_, b_ = secondary_rays(top, bot, tv, sun)
    return _ops().ray_visibility(net.op_model(), t_, b_, tv, 2).cpu().reshape(top.shape[0], tv.numel())


def check_sums(out, ex, V, PS, S):
    R = out.shape[0]
    E, V, PS = ex.double(), V[:R * S].cpu().reshape(R, S), PS[:R * S].cpu().reshape(R, S)
    e5, v5 = ex > .5, V > .5
    for k, m in enumerate((e5 & v5, e5, v5)):
        assert torch.equal(out[:, k].double(), m.sum(1).double()), f"slot {k}: {out[:, k].tolist()} against {m.sum(1).tolist()}"
    terms = (E * PS.double(), V.double() * PS.double(), PS.double(), (E - V.double()) ** 2, (E - V.double()).abs())      # float64, of the fp32 values
    for k, t64 in enumerate(terms):
        bound = 2 * (S + 2) * 2.0 ** -24 * t64.abs().sum(1)
        err = (out[:, 3 + k].double() - t64.sum(1)).abs()
        assert bool((err <= bound).all()), f"slot {3 + k}: off by {float(err.max()):.3e}, allowed {float(bound[err.argmax()]):.3e}"


def check_kernel(net, W, R, S, seed):
    from season_nerf_amd.evaluator import sample_parameters_on
    top, bot = view_rays(R, seed)
    tv = sample_parameters_on(torch.device(DEV), S, eval_mode=True, include_end_pt=True)
    V, PS = v_and_ps(R, S, seed)
    coincide = S % (2 if W == 512 else 4) == 0
    for sun in SUNS:
        rv = ray_visibility(net, top, bot, tv, sun)
        full, ex_full = audit_call(net, top, bot, tv, sun, V, PS, 2 | 4)
        walked = rv >= SAT if S > 32 else torch.ones_like(rv, dtype=torch.bool)
        assert torch.equal(ex_full[walked], rv[walked]), f"W={W} R={R} S={S}: Exact_Solar differs in bits from ray_visibility on {int((ex_full[walked] != rv[walked]).sum())} samples"
        assert bool((ex_full[~walked] < SAT).all())
        check_sums(full, ex_full, V, PS, S)
        early, ex_early = audit_call(net, top, bot, tv, sun, V, PS, 2)
        if coincide:
            assert torch.equal(ex_early, rv), f"W={W} R={R} S={S}: early-out groups coincide, Exact_Solar differs in bits from ray_visibility"
        assert bool(((ex_early - ex_full).abs() <= 2 * SAT).all())
        check_sums(early, ex_early, V, PS, S)
        again, ex_again = audit_call(net, top, bot, tv, sun, V, PS, 2)
        assert torch.equal(again, early) and torch.equal(ex_again, ex_early), "two launches differ"
        print(f"  W={W} R={R} S={S} sun_z={sun[2]}: {int((~walked).sum())} of {R * S} samples cut short by ray_visibility's early-out; in the sun {int((ex_full > .5).sum())}; "
              f"skipped by the audit's early-out {int((ex_early != ex_full).sum())}")


@pytest.mark.parametrize("S", S_ALL)
@pytest.mark.parametrize("W", [64, 256, 512])
def test_kernel_vs_ray_visibility(golden_dir, W, S):
    check_kernel(net_of(golden_dir, f"sharp_W{W}"), W, 5, S, 100 * W + S)


@pytest.mark.parametrize("R,S", [(1, 33), (2, 5), (2, 96)])
@pytest.mark.parametrize("W", [64, 256, 512])
def test_kernel_few_rays(golden_dir, W, R, S):
    check_kernel(net_of(golden_dir, f"sharp_W{W}"), W, R, S, 7 * W + R)


@pytest.mark.parametrize("W", [64, 512])
def test_persistent_loop(golden_dir, W):
    """More primary rays than workgroups: every row written, nothing around them, and the first rows the same as in a launch of those rays alone."""
    from season_nerf_amd.evaluator import sample_parameters_on
    net = net_of(golden_dir, f"sharp_W{W}")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    R, S = n_cu + 37, 8
    top, bot = view_rays(R, W)
    tv = sample_parameters_on(torch.device(DEV), S, eval_mode=True, include_end_pt=True)
    V, PS = v_and_ps(R, S, W)
    a, xa = audit_call(net, top, bot, tv, SUNS[0], V, PS, 2)
    b, xb = audit_call(net, top, bot, tv, SUNS[0], V, PS, 2)
    assert torch.equal(a, b) and torch.equal(xa, xb)
    check_sums(a, xa, V, PS, S)
    assert torch.equal(xa, ray_visibility(net, top, bot, tv, SUNS[0]))      # S = 8: one pass, groups coincide
    c, xc = audit_call(net, top, bot, tv, SUNS[0], V, PS, 2, n=37)
    assert torch.equal(c, a[:37]) and torch.equal(xc, xa[:37])


def test_op(golden_dir):
    """The op equals the C call; opcheck (schema and fake kernel); argument errors."""
    import season_nerf_amd as sn
    from season_nerf_amd.evaluator import sample_parameters_on
    ops = sn.ops.load()
    net = net_of(golden_dir, "sharp_W64")
    h = net.device_model()
    R, S = 5, 40
    top, bot = view_rays(R, 3)
    tv = sample_parameters_on(torch.device(DEV), S, eval_mode=True, include_end_pt=True)
    V, PS = v_and_ps(R, S, 3)
    V, PS = V[:R * S].reshape(R, S).contiguous(), PS[:R * S].reshape(R, S).contiguous()
    sun = [float(x) for x in SUNS[0]]
    out, ex = ops.solar_audit(h, top, bot, tv, sun, V, PS, 2, True)
    c_out, c_ex = audit_call(net, top, bot, tv, SUNS[0], V, PS, 2)
    assert out.shape == (R, 8) and ex.shape == (R, S) and out.dtype == torch.float32 and out.device == top.device
    assert torch.equal(out.cpu(), c_out) and torch.equal(ex.cpu(), c_ex)
    out2, ex2 = ops.solar_audit(h, top, bot, tv, sun, V, PS, 2, False)
    assert torch.equal(out2, out) and ex2.numel() == 0
    o0, x0 = ops.solar_audit(h, top[:0], bot[:0], tv, sun, V[:0], PS[:0], 0, True)
    assert o0.shape == (0, 8) and x0.shape == (0, S)
    for want in (True, False):
        torch.library.opcheck(torch.ops.season_nerf.solar_audit.default, (h, top, bot, tv, sun, V, PS, 2, want), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError, match="top"):
        ops.solar_audit(h, top[:, :2].contiguous(), bot, tv, sun, V, PS, 0, False)
    with pytest.raises(RuntimeError, match="bot"):
        ops.solar_audit(h, top, bot[:3], tv, sun, V, PS, 0, False)
    with pytest.raises(RuntimeError, match="tvals"):
        ops.solar_audit(h, top, bot, tv.reshape(1, -1), sun, V, PS, 0, False)
    with pytest.raises(RuntimeError, match="sun"):
        ops.solar_audit(h, top, bot, tv, sun[:2], V, PS, 0, False)
    with pytest.raises(RuntimeError, match="sun"):
        ops.solar_audit(h, top, bot, tv, [sun[0], sun[1], 0.0], V, PS, 0, False)
    with pytest.raises(RuntimeError, match="sun"):
        ops.solar_audit(h, top, bot, tv, [float("nan"), sun[1], sun[2]], V, PS, 0, False)
    with pytest.raises(RuntimeError, match="est_vis"):
        ops.solar_audit(h, top, bot, tv, sun, V[:3], PS, 0, False)
    with pytest.raises(RuntimeError, match="ps"):
        ops.solar_audit(h, top, bot, tv, sun, V, PS.double(), 0, False)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.solar_audit(h, top, bot, tv, sun, V.cpu(), PS, 0, False)
    with pytest.raises(RuntimeError, match="flags"):
        ops.solar_audit(h, top, bot, tv, sun, V, PS, 8, False)
    with pytest.raises(RuntimeError, match="NULL"):
        ops.solar_audit(0, top, bot, tv, sun, V, PS, 0, False)
    net8 = net_of(golden_dir, "init_W64_s2", "i8x3")
    with pytest.raises(RuntimeError, match="snerf_field_solar_audit"):
        ops.solar_audit(net8.device_model(), top, bot, tv, sun, V, PS, 0, False)
    with pytest.raises(ValueError, match="solar_audit"):
        sn.solar_audit(net, top, bot[:3], SUNS, S)
    with pytest.raises(ValueError, match="sun_z"):
        sn.solar_audit(net, top, bot, -SUNS, S)


def test_two_walk_chunks(golden_dir):
    """M = 33 sun directions (two chunks of the sun walk) give what the suns give one at a time, bit for bit, Exact_Solar included."""
    import season_nerf_amd as sn
    net = net_of(golden_dir, "sharp_W64")
    top, bot = view_rays(6, 11)
    rng = np.random.Generator(np.random.PCG64(5))
    el, az = np.deg2rad(rng.uniform(20, 80, 33)), rng.uniform(0, 2 * np.pi, 33)
    suns = np.stack([np.cos(el) * np.sin(az), np.cos(el) * np.cos(az), np.sin(el)], 1)
    a = sn.solar_audit(net, top, bot, suns, 8, want_exact=True)
    assert a.sums.shape == (33, 6, 8) and a.sums.dtype == torch.float64 and a.n_samples == 8 and len(a) == 33
    total = {f: {k: 0 for k in ("TP", "TN", "FP", "FN")} for f in ("All_Solar_Vis", "Surface_Solar_Vis")}
    for j in (0, 1, 31, 32):
        one = sn.solar_audit(net, top, bot, suns[j:j + 1], 8, want_exact=True)
        assert torch.equal(one.sums[0], a.sums[j]) and torch.equal(one.exact(0), a.exact(j)), j
        assert one.confusion() == a.confusion(j) == one.confusion(0)
    for j in range(33):
        c = a.confusion(j)
        assert sum(c["All_Solar_Vis"].values()) == 6 * 8 and sum(c["Surface_Solar_Vis"].values()) == 6
        for f in total:
            for k in total[f]:
                total[f][k] += c[f][k]
    assert a.confusion() == total
    with pytest.raises(ValueError, match="want_exact"):
        sn.solar_audit(net, top, bot, suns[:1], 8).exact(0)


# ------------------------------------------------------------------------------------------------ against the reference's fixture
def _render(golden_dir, g, tag, S, vi, si, precision="bf16x3"):
    import season_nerf_amd as sn
    net = net_of(golden_dir, tag, precision)
    H, Wd = (int(x) for x in g["lattice"])
    return sn.component_render_by_dir(net, VIEWS[vi], SUN_EL_AZ[si], 0.0, (H, Wd, S), g["W2C"], g["W2L_H"], DEV, include_exact_solar=True, skip_weightless=None)


def _deviation(d, g, k):
    """A device render against the recorded per-sample arrays -> max |Exact - recorded|, max |Est - recorded|, max over rays |sum vis PS - recorded's|."""
    ex, es = d["Exact_Solar"][..., 0], d["Est_Solar_Vis"][..., 0]
    ps = ps_of(d["Rho"][..., 0], d["Deltas"][..., 0])
    _, _, _, se, sv = reference_of(g, k, BAND, BAND_SURF)
    return (float(np.abs(ex - g[k + "_Exact_Solar"]).max()), float(np.abs(es - g[k + "_Est_Solar_Vis"]).max()),
            float(max(np.abs((ex * ps).sum(1) - se).max(), np.abs((es * ps).sum(1) - sv).max())))


def test_per_sample_deviation(golden_dir):
    """The measurement behind E_EXACT, E_EST, E_SURF and the bands of test_audit_host.py: `component_render_by_dir(include_exact_solar=True)` on the device -
    code the audit does not run - against the reference's recorded per-sample arrays, over every render the fixture holds per sample."""
    g = fixture(golden_dir)
    worst = {"exact": (0.0, ""), "est": (0.0, ""), "surf": (0.0, "")}
    for tag, S, vi, si in sorted(ARRAYS):
        k = key_of(tag, S, vi, si)
        dev = _deviation(_render(golden_dir, g, tag, S, vi, si), g, k)
        print(f"  {k}: max |Exact_Solar - recorded| {dev[0]:.4e}   max |Est_Solar_Vis - recorded| {dev[1]:.4e}   max |sum vis PS - recorded's| {dev[2]:.4e}")
        for name, v in zip(("exact", "est", "surf"), dev):
            if v > worst[name][0]:
                worst[name] = (v, k)
    print(f"  E_EXACT = {worst['exact'][0]:.4e} ({worst['exact'][1]})   E_EST = {worst['est'][0]:.4e} ({worst['est'][1]})   E_SURF = {worst['surf'][0]:.4e} "
          f"({worst['surf'][1]})   (recorded: {E_EXACT:.4e}, {E_EST:.4e}, {E_SURF:.4e})")
    assert worst["exact"][0] <= E_EXACT and worst["est"][0] <= E_EST and worst["surf"][0] <= E_SURF, "the recorded maxima no longer bound the render path's deviation"


def _check_against_fixture(g, k, conf, band, band_surf, ps_exact=None, ps_est=None):
    ref, n_band, n_surf, se, sv = reference_of(g, k, band, band_surf)
    for fam, allowed in (("All_Solar_Vis", n_band), ("Surface_Solar_Vis", n_surf)):
        for key in ("TP", "TN", "FP", "FN"):
            assert abs(conf[fam][key] - ref[fam][key]) <= allowed, (k, fam, key, conf[fam][key], ref[fam][key], allowed)
    if ps_exact is not None:
        assert np.abs(ps_exact - se).max() <= band_surf, (k, "sum Exact PS", float(np.abs(ps_exact - se).max()))
        assert np.abs(ps_est - sv).max() <= band_surf, (k, "sum Est PS", float(np.abs(ps_est - sv).max()))
    return ref, n_band, n_surf


@pytest.mark.parametrize("S", S_LIST)
@pytest.mark.parametrize("tag", TAGS)
def test_audit_by_dir_vs_reference(golden_dir, tag, S):
    """`audit_by_dir` against the recorded arrays: every confusion count within the number of recorded samples (rays, for the surface counts) inside the
    band, sum Exact PS and sum Est PS per ray within BAND_SURF of the float64 sums of the recorded arrays."""
    import season_nerf_amd as sn
    g = fixture(golden_dir)
    net = net_of(golden_dir, tag)
    assert net.resolved_precision == "bf16x3"
    H, Wd = (int(x) for x in g["lattice"])
    for vi in range(len(VIEWS)):
        a = sn.audit_by_dir(net, VIEWS[vi], SUN_EL_AZ, (H, Wd, S), g["W2C"], g["W2L_H"], DEV)
        assert a.sums.shape == (len(SUN_EL_AZ), H * Wd, 8)
        for si in range(len(SUN_EL_AZ)):
            k = key_of(tag, S, vi, si)
            conf = a.confusion(si)
            ref, n_band, n_surf = _check_against_fixture(g, k, conf, BAND, BAND_SURF, a.ps_exact[si].cpu().numpy(), a.ps_est[si].cpu().numpy())
            print(f"  {k}: All {conf['All_Solar_Vis']} (reference {ref['All_Solar_Vis']}, {n_band} samples in the band)  Surface {conf['Surface_Solar_Vis']} "
                  f"(reference {ref['Surface_Solar_Vis']}, {n_surf} rays in the band)")


def test_eval_solar_data_on_device_dict(golden_dir):
    """`eval_solar_data` on an ImgDict that still has its device tensors counts on the device: the same integers as on the dict's float64 arrays on the
    host, and the recorded ones within the band."""
    import season_nerf_amd as sn
    g = fixture(golden_dir)
    for tag, S, vi, si in (("sharp_W64", 40, 1, 0), ("sharp_W256", 96, 1, 2)):
        d = _render(golden_dir, g, tag, S, vi, si)
        assert d.dev is not None
        on_dev = sn.eval_solar_data(d)
        on_host = sn.eval_solar_data({k2: d[k2] for k2 in ("Exact_Solar", "Est_Solar_Vis", "Rho", "Deltas")})
        assert on_dev == on_host, (on_dev, on_host)
        _check_against_fixture(g, key_of(tag, S, vi, si), on_dev, BAND, BAND_SURF)


def test_fallback_int8(golden_dir):
    """A network the kernels do not serve (resolved to int8 digits) gets the audit from `forward_Solar` on the sample points, `_exact_solar_visibility` and
    float64 sums: against the fixture at that path's own measured band - twice the int8 render path's deviation from the recorded per-sample arrays,
    measured here on the same renders."""
    import season_nerf_amd as sn
    from season_nerf_amd import render as R_
    g = fixture(golden_dir)
    tag, S, vi = "init_W64_s2", 40, 0
    net = net_of(golden_dir, tag, "i8x3")
    assert net.resolved_precision == "i8x3" and not R_._walks(net)
    H, Wd = (int(x) for x in g["lattice"])
    suns = [si for si in range(len(SUN_EL_AZ)) if (tag, S, vi, si) in ARRAYS]
    assert len(suns) == 2
    a = sn.audit_by_dir(net, VIEWS[vi], [SUN_EL_AZ[si] for si in suns], (H, Wd, S), g["W2C"], g["W2L_H"], DEV, want_exact=True)
    for j, si in enumerate(suns):
        k = key_of(tag, S, vi, si)
        e_x, e_v, e_s = _deviation(_render(golden_dir, g, tag, S, vi, si, "i8x3"), g, k)
        print(f"  {k}: the int8 render path stands {max(e_x, e_v):.3e} per sample and {e_s:.3e} per ray from the recorded arrays")
        assert 2 * max(e_x, e_v) <= 0.05, "the band says nothing"
        _check_against_fixture(g, k, a.confusion(j), 2 * max(e_x, e_v), 2 * e_s, a.ps_exact[j].cpu().numpy(), a.ps_est[j].cpu().numpy())
        assert np.abs(a.exact(j).cpu().numpy().astype(np.float64) - g[k + "_Exact_Solar"]).max() <= 2 * e_x


def test_advanced_solar(golden_dir):
    """`advanced_solar` on small grids: the reference's `Full_ans` structure, every cell the confusion of `audit_by_dir` for that view and sun, the key of
    the second index holding the elevations; `_shadow_analyasis` runs on it."""
    import season_nerf_amd as sn
    from season_nerf_amd.solar_audit import _BASE_KEYS, _shadow_analyasis
    g = fixture(golden_dir)
    net = net_of(golden_dir, "sharp_W64")
    size = (6, 7, 12)
    sat_az, sat_el, sun_az, sun_el = [30.0, 200.0], [60.0, 80.0, 85.0], [75.0, 320.0], [20.0, 70.0]
    full = sn.advanced_solar(net, g["W2C"], g["W2L_H"], DEV, size, sat_thetas=sat_az, sat_el_phis=sat_el, solar_thetas=sun_az, solar_el_phis=sun_el)
    assert list(full) == ["All_Solar_Vis", "Surface_Solar_Vis", "Keys"]
    assert list(full["Keys"]) == ["Idx_1_sat_azmuth", "Idx_2_sat_el", "Idx_3_solar_azmuth", "Idx_4_solar_el"]
    assert np.array_equal(full["Keys"]["Idx_2_sat_el"], sat_el) and np.array_equal(full["Keys"]["Idx_1_sat_azmuth"], sat_az)
    for fam, total in (("All_Solar_Vis", 6 * 7 * 12), ("Surface_Solar_Vis", 6 * 7)):
        assert list(full[fam]) == ["TP", "TN", "FP", "FN"] and all(full[fam][k].shape == (2, 3, 2, 2) for k in full[fam])
        assert full[fam]["TP"].dtype.kind == "i" and full[fam]["TN"].dtype == np.float64
        assert np.array_equal(sum(full[fam][k] for k in full[fam]), np.full((2, 3, 2, 2), total))
    for i, j, k, ell in ((0, 0, 0, 0), (1, 2, 1, 0), (0, 1, 1, 1)):
        one = sn.audit_by_dir(net, [sat_el[j], sat_az[i]], [[sun_el[ell], sun_az[k]]], size, g["W2C"], g["W2L_H"], DEV).confusion(0)
        for fam in one:
            assert {key: int(full[fam][key][i, j, k, ell]) for key in one[fam]} == one[fam], (i, j, k, ell, fam)
    out = _shadow_analyasis({"Region": full})
    assert out["Region"]["All_Solar_Vis"]["Accuracy"].shape == (2, 3, 2, 2) and list(out["Region"]["Surface_Solar_Vis"]["Overall"]) == _BASE_KEYS
