"""CPU checks behind tests/test_gpu_loss_all.py: the closed float64 forms of tests/loss_all_cases.py against torch.autograd in float64 on
season_nerf_amd/adaptive_loss.py itself (alpha and scale as leaves), the conditions that keep the alpha set honest, and the argument errors of
snerf_loss_all_forward / _backward (refused before any launch: no GPU is needed to be refused).

Conditions on the cases (E_ref = the float32 evaluation of adaptive_loss.py against its float64 evaluation on the same float32 inputs):
  * alpha-gradients: E_ref at most 1e-3 of the gradient's largest magnitude;  values, input gradients, scale gradients: E_ref at most 1e-5 of theirs -
    a tolerance built on E_ref (train_kernel_cases.tolerance) then means something.  Measured on the CPU for these cases: 2.4e-4 and 1.9e-6 at the worst;
  * mutation: a reference without the derivative of b = |alpha - 2| + eps misses that tolerance by at least 10x in every case with alpha != 2 - except one
    ulp below 2, where d = alpha + eps is exactly 2, rho = z / 2 does not depend on b at all and the two b' terms cancel identically (asserted: the mutant
    equals the reference there to 1e-9).  A second mutant, b treated as a constant inside u = 1 + z / b only, is caught in every case with alpha != 2,
    that one included (it moves the gradient by 0.2 ... 1e9).
The closed form itself must agree with float64 autograd to 1e-9 of the quantity's largest magnitude (both are float64 evaluations of one formula: sums of
up to 2.2e5 terms, each to a few ulp of 1.1e-16)."""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_all_cases as lc
import train_kernel_cases as tk


@pytest.mark.parametrize("D,scale,rows", lc.HOST_CASES, ids=[f"D{d}-c{c}-M{m}" for d, c, m in lc.HOST_CASES])
def test_closed_forms_against_autograd_and_case_conditions(D, scale, rows):
    x = lc.residuals(tk.rng_for(f"nll-{D}-{scale}-{rows}"), rows, D)
    for alpha in lc.ALPHAS:
        a, c = np.float32([alpha] * D), np.float32([scale] * D)
        v, dx, da, dc = lc.nll_closed(x, a, c)
        v64, dx64, da64, dc64 = lc.nll_autograd(x, a, c, torch.float64)
        v32, dx32, da32, dc32 = lc.nll_autograd(x, a, c, torch.float32)
        for name, got, want in (("value", v, v64), ("d_x", dx, dx64), ("d_alpha", da, da64), ("d_scale", dc, dc64)):
            err, mag = np.abs(np.asarray(got) - want).max(), np.abs(want).max()
            assert err <= 1e-9 * max(mag, 1e-30), (alpha, name, err, mag)
        e_a = np.abs(da32 - da64).max()
        # each as a fraction of the quantity's largest magnitude, like the alpha-gradient's (a mean nll of 800 at c = 0.0101 has a float32 ulp of 6e-5)
        e_rest = {"value": abs(v32 - v64) / abs(v64), "d_x": np.abs(dx32 - dx64).max() / np.abs(dx64).max(), "d_scale": np.abs(dc32 - dc64).max() / np.abs(dc64).max()}
        print(f"FIG D={D} c={scale} alpha={alpha!r}: E_ref d_alpha {e_a:.2e} of {np.abs(da64).max():.2e}; " + ", ".join(f"{k} {e:.2e}" for k, e in e_rest.items()))
        assert e_a <= 1e-3 * np.abs(da64).max(), (alpha, e_a, da64)
        for k, e in e_rest.items():
            assert e <= 1e-5, (alpha, k, e)
        if alpha != 2.0:
            tol = tk.tolerance(e_a, np.abs(da64))
            mutant = lc.nll_closed(x, a, c, drop_db=True)[2]
            inner = lc.nll_closed(x, a, c, drop_db="inner")[2]
            print(f"FIG   mutants: without b' {np.abs(mutant - da64).min():.2e}, without b' inside u {np.abs(inner - da64).min():.2e}, tolerance {tol.max():.2e}")
            assert (np.abs(inner - da64) >= 10 * tol).all(), (alpha, inner, da64, tol)
            if np.float32(alpha) + np.float32(lc.EPS) == np.float32(2):
                # one ulp below 2: d = alpha + eps is exactly 2, so rho = (b / 2)((1 + z / b) - 1) = z / 2 whatever b is - the two b' terms cancel
                # identically and NO reference can tell whether they are there; the mutant that keeps one of them (above) still can
                assert (np.abs(mutant - da64) <= 1e-9 * np.abs(da64)).all(), (alpha, mutant, da64)
            else:
                assert (np.abs(mutant - da64) >= 10 * tol).all(), (alpha, mutant, da64, tol)


def test_reference_matches_the_closed_forms_and_the_key_order():
    """loss_all_cases.reference (what the GPU test compares with) gives the adaptive terms of the closed form, and the key order and weights get_loss has"""
    h = lc.make_inputs("ref", 257, 131, 7, 1.3)
    for name, flags in lc.CONFIGS.items():
        g = np.linspace(0.5, 1.5, len(lc.NAMES[flags & 3]))
        vals, wts, scale, grads = lc.reference(h, flags, torch.float64, g)
        names = lc.NAMES[flags & 3]
        assert len(vals) == len(names) and (scale >= np.abs(vals) * (1 - 1e-12)).all()
        if flags & lc.ADAPTIVE:
            v, dx, da, dc = lc.nll_closed(h["rgb"].astype(np.float64) - h["gt"].astype(np.float64), h["alpha_c"], h["scale_c"])
            i = names.index("Color_ada")
            assert abs(vals[i] - v) <= 1e-12 * abs(v)
            np.testing.assert_allclose(grads["alpha_c"].reshape(-1), g[i] * da, rtol=1e-9)
            np.testing.assert_allclose(grads["scale_c"].reshape(-1), g[i] * dc, rtol=1e-9)
            np.testing.assert_allclose(grads["rgb"], g[i] * dx, rtol=1e-9, atol=1e-18)
            width = np.float64(h["scale_c"]).mean()
            assert wts[0] == pytest.approx(0.03 / width ** 2, rel=1e-12) and wts[1] == wts[0] and wts[2] == 0.03
            assert grads["rgb_merged"] is None or not grads["rgb_merged"].any()           # `Color` is a value only beside the adaptive loss
        else:
            assert names == ("Solar_Correction", "Solar_Correction_2", "Sky_Color_Var", "Albedo_Color", "Color") + (("Alpha_Adjust",) if flags & lc.PRIOR else ())
            on, off = ("rgb_merged", "rgb") if flags & lc.PRIOR else ("rgb", "rgb_merged")          # `Color` is formed on the merged colour in the prior phase
            assert grads[on].any() and (grads[off] is None or not grads[off].any())
            assert list(wts[:4]) == [0.03] * 4 and wts[4] == 1.0
        assert (grads["sky"] is None or not grads["sky"].any()) == bool(flags & lc.SKY_DETACHED)
        if flags & lc.PRIOR:
            assert grads["pe"].any()


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    import os
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("snerf_build", os.path.join(repo, "season_nerf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    b.build_ops()
    import season_nerf_amd as sn
    return sn._lib.lib()


def test_loss_all_entry_points_refuse_before_any_launch(lib):
    """snerf_loss_all_forward / _backward / _term_count check every argument before any HIP call: no pointer is read, so any non-null address will do"""
    from season_nerf_amd._lib import LossIn, LossGrads
    buf = np.zeros(64, dtype=np.float32)
    a = buf.ctypes.data
    assert lib.snerf_loss_all_scratch_bytes() >= 1024 * (17 * 8 + 3 * 8)
    assert [lib.snerf_loss_all_term_count(f) for f in (1, 3, 2, 5, 7, 6)] == [8, 12, 6, 8, 12, 6]
    assert [lib.snerf_loss_all_term_count(f) for f in (0, 4)] == [5, 5]
    for f in (8, -1):
        assert lib.snerf_loss_all_term_count(f) == -1 and b"flags" in lib.snerf_last_error()

    def full(flags=3, **kw):
        i = LossIn(n_rays=8, n_solar_rays=8, n_samples=4, flags=flags, world=1, w_solar=.03, w_color=1., w_alpha=1.)
        for name, _ in LossIn._fields_:
            if name.startswith("d_") and name != "d_albedo_min_global":
                setattr(i, name, a)
        for k, v in kw.items():
            setattr(i, k, v)
        return i

    def grads(**kw):
        o = LossGrads(*[a] * 10)
        for k, v in kw.items():
            setattr(o, k, v)
        return o

    fwd = lambda i, scratch=a, vals=a, wts=a, aux=a: lib.snerf_loss_all_forward(C.byref(i) if i is not None else None, scratch, vals, wts, aux, None)
    bwd = lambda i, o, aux=a, g=a: lib.snerf_loss_all_backward(C.byref(i) if i is not None else None, aux, g, C.byref(o) if o is not None else None, None)
    refused = []

    def check(rc, word):
        assert rc == -1 and word.encode() in lib.snerf_last_error(), (rc, word, lib.snerf_last_error())
        refused.append(word)

    check(fwd(None), "NULL input")
    check(fwd(full(flags=8)), "flags")
    for f in (0, 4):      # the MSE free phase is a served configuration: the call gets as far as its outputs, with no pointer of the other configurations
        none = {k: None for k in ("d_rgb_merged", "d_pe", "d_pe_supervised", "d_alpha_color", "d_scale_color", "d_alpha_alpha", "d_scale_alpha", "d_logz_value", "d_logz_slope")}
        assert fwd(full(flags=f, **none), scratch=None) == -1 and b"NULL scratch" in lib.snerf_last_error()
    for k in ("n_rays", "n_solar_rays", "n_samples", "world"):
        check(fwd(full(**{k: 0})), "counts")
    check(fwd(full(n_rays=1 << 31)), "counts")
    for k in ("d_rgb", "d_gt", "d_albedo", "d_sky", "d_solar_vis", "d_pv_exact", "d_pe_solar"):
        check(fwd(full(**{k: None})), "NULL image-ray or sun-ray")
    for k in ("d_alpha_color", "d_scale_color", "d_logz_value", "d_logz_slope"):
        check(fwd(full(flags=1, **{k: None})), "adaptive colour loss needs")
        assert fwd(full(flags=2, **{k: None}), scratch=None) == -1 and b"NULL scratch" in lib.snerf_last_error()      # not needed without the adaptive loss
    for k in ("d_pe", "d_pe_supervised"):
        check(fwd(full(flags=2, **{k: None})), "prior phase needs")
    for k in ("d_alpha_alpha", "d_scale_alpha"):
        check(fwd(full(flags=3, **{k: None})), "alpha loss object")
    check(fwd(full(w_solar=float("nan"))), "NaN weight")
    for k in ("scratch", "vals", "wts", "aux"):
        check(fwd(full(), **{k: None}), "NULL scratch or output")
    check(bwd(None, grads()), "NULL input")
    check(bwd(full(), None), "NULL aux")
    check(bwd(full(), grads(), aux=None), "NULL aux")
    check(bwd(full(), grads(), g=None), "NULL aux")
    for k in ("d_g_rgb", "d_g_albedo", "d_g_sky", "d_g_solar_vis", "d_g_rgb_merged", "d_g_pe", "d_g_alpha_color", "d_g_scale_color", "d_g_alpha_alpha", "d_g_scale_alpha"):
        check(bwd(full(), grads(**{k: None})), "NULL gradient output")
    assert len(refused) == 41
