"""CPU-only checks of the solar audit (the reference's mg_Advanced_Solar.py study scored inside the field kernel): the C ABI's argument check, the three
kernels in the shipped code objects, the `solar_audit.npz` fixture against the CPU oracle, the mirrors of the reference's functions against its recorded
results, and the conditions the comparison bands of tests/test_gpu_audit.py have to meet on that fixture.

The fixture.  The reference's 48 renders (4 weight sets x 2 sample counts x 2 views x 3 suns on a 10 x 12 lattice) are 2.9 MB per sample; the fixture may not
be larger than shadow_points.npz.  It holds the confusion dicts and statistics of all 48, the per-sample arrays of the nine renders of `ARRAYS`, and for the
other 39 the per-ray sums and the samples near .5 that the comparisons read (tools/make_solar_audit_golden.py).

The bands.  Measured on an MI355X with the path the feature does not touch (`component_render_by_dir(include_exact_solar=True)` on the device), over every
render the fixture holds per sample, printed by
    python -m pytest tests/test_gpu_audit.py -m gpu -k per_sample_deviation -s
E_EXACT = max |Exact_Solar - recorded|, E_EST = max |Est_Solar_Vis - recorded|, E_SURF = max over rays |sum_s vis PS - the same of the recorded arrays|
(vis = Exact and Est).  BAND = 2 max(E_EXACT, E_EST): a recorded sample whose exact or learned visibility lies within BAND of .5 may be counted on either
side by the device; BAND_SURF = 2 E_SURF likewise for a ray's sum vis PS against .3.  The factor 2 covers the kernel's different summation order (as in
test_shadow_host.py)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc
from test_isa_guards import _device_code_objects, _kernel_metadata
from test_surface_host import TAGS, built, weights      # noqa: F401  (built: the session fixture)

E_EXACT = 1.46e-4    # measured 1.4561e-04 (sharp_W256, S = 40, view 0, sun 0), rounded up
E_EST = 2.99e-5      # measured 2.9862e-05 (sharp_W256, S = 40, view 0, sun 2), rounded up
E_SURF = 6.11e-5     # measured 6.1001e-05 (sharp_W64, S = 40, view 1, sun 2), rounded up
BAND = 2 * max(E_EXACT, E_EST)
BAND_SURF = 2 * E_SURF

S_LIST = (40, 96)
VIEWS = ((60.0, 30.0), (80.0, 200.0))                       # (el, az) in degrees
SUN_EL_AZ = ((20.0, 75.0), (45.0, 190.0), (70.0, 320.0))    # (el, az) in degrees
STAT_KEYS = ("Acc", "Acc_Balanced", "Shadow_Prev", "Prec_P", "Recall_P", "Prec_N", "Recall_N", "F1_P", "F1_N")
CONF_KEYS = ("TP", "TN", "FP", "FN")
FAMILIES = ("All_Solar_Vis", "Surface_Solar_Vis")


def key_of(tag, S, vi, si=None):
    return f"{tag}_S{S}_v{vi}" + ("" if si is None else f"_s{si}")


def renders():
    """Every render of the fixture: weight set x sample count x view x sun, in the order of the fixture's stacked arrays."""
    for tag in TAGS:
        for S in S_LIST:
            for vi in range(len(VIEWS)):
                for si in range(len(SUN_EL_AZ)):
                    yield tag, S, vi, si, key_of(tag, S, vi, si)


# The renders recorded per sample (all 48 would be 2.9 MB): every weight set at S = 40 on one view (the views alternate) under the lowest and the highest
# sun, and one at S = 96.  The others carry their confusion dicts, statistics, per-ray sums and the samples within NEAR of .5 (tools/make_solar_audit_golden.py).
ARRAYS = frozenset([(tag, 40, i % 2, si) for i, tag in enumerate(TAGS) for si in (0, 2)] + [("sharp_W64", 96, 1, 0)])
NEAR = 1e-3


class Fixture(dict):
    """solar_audit.npz with the arrays that do not depend on the sun (Rho, Deltas) found under every sun's key."""

    def __missing__(self, k):
        for name in ("_Rho", "_Deltas"):
            if k.endswith(name) and "_s" in k.rsplit("_v", 1)[1]:
                return self[k[:-len(name)].rsplit("_s", 1)[0] + name]
        raise KeyError(k)


def fixture(golden_dir):
    return as_fixture(np.load(os.path.join(golden_dir, "solar_audit.npz"), allow_pickle=False))


def as_fixture(arrays):
    """The arrays of solar_audit.npz with every render's rows of the stacked arrays under the render's own key."""
    g = Fixture(arrays)
    assert list(g["tags"]) == TAGS and tuple(int(s) for s in g["S_list"]) == S_LIST
    assert np.array_equal(g["views"], np.array(VIEWS)) and np.array_equal(g["sun_el_az"], np.array(SUN_EL_AZ))
    for i, (tag, S, vi, si, k) in enumerate(renders()):
        assert ((k + "_Exact_Solar") in g) == ((tag, S, vi, si) in ARRAYS) and bool(np.isnan(g["surf"][i]).all()) == ((tag, S, vi, si) in ARRAYS), k
        g[k + "_confusion"], g[k + "_stats"] = g["confusion"][i], g["stats"][i]
        if (tag, S, vi, si) not in ARRAYS:
            g[k + "_surf"], g[k + "_near"] = g["surf"][i], g["near"][:, int(g["near_start"][i]):int(g["near_start"][i + 1])]
    return g


def ps_of(rho, deltas):
    """PS as eval_solar_data forms it (mg_Advanced_Solar.py:23-24) from [R,S] arrays, in their dtype (float64 in the reference)."""
    y = rho * deltas
    pv = np.exp(-np.cumsum(np.concatenate([np.zeros_like(y[:, :1]), y], 1), 1))[:, :-1]
    return pv * (1 - np.exp(-y))


def confusion_of_arrays(exact, est, ps):
    """The two confusion dicts of eval_solar_data from [R,S] arrays, restated."""
    ex, es = exact.astype(np.float64), est.astype(np.float64)
    gt, et = ex > .5, es > .5
    gs, ets = (ex * ps).sum(1) > .3, (es * ps).sum(1) > .3
    c = lambda m: int(m.sum())
    return {"All_Solar_Vis": {"TP": c(gt & et), "TN": c(~gt & ~et), "FP": c(~gt & et), "FN": c(gt & ~et)},
            "Surface_Solar_Vis": {"TP": c(gs & ets), "TN": c(~gs & ~ets), "FP": c(~gs & ets), "FN": c(gs & ~ets)}}


def recorded_confusion(g, k):
    return {fam: dict(zip(CONF_KEYS, (int(x) for x in g[k + "_confusion"][i]))) for i, fam in enumerate(FAMILIES)}


def in_band(exact, est, band):
    """Recorded samples whose exact or learned visibility lies within `band` of .5 -> bool, the arrays' shape."""
    return (np.abs(exact.astype(np.float64) - .5) <= band) | (np.abs(est.astype(np.float64) - .5) <= band)


def reference_of(g, k, band, band_surf):
    """What the comparisons need of a recorded render -> (confusion dicts, number of samples inside `band`, number of rays inside `band_surf`,
    sum Exact PS [R], sum Est PS [R]): from the per-sample arrays where the fixture has them, else from `_near` and `_surf`."""
    if (k + "_Exact_Solar") in g:
        ex, es = g[k + "_Exact_Solar"].astype(np.float64), g[k + "_Est_Solar_Vis"].astype(np.float64)
        ps = ps_of(g[k + "_Rho"].astype(np.float64), g[k + "_Deltas"].astype(np.float64))
        n_band, se, sv = int(in_band(ex, es, band).sum()), (ex * ps).sum(1), (es * ps).sum(1)
    else:
        assert band <= NEAR, "the fixture records the samples within NEAR of .5 only"
        near = g[k + "_near"].astype(np.float64)
        n_band, (se, sv) = int(((near[0] <= band) | (near[1] <= band)).sum()), g[k + "_surf"]
    n_surf = int(((np.abs(se - .3) <= band_surf) | (np.abs(sv - .3) <= band_surf)).sum())
    return recorded_confusion(g, k), n_band, n_surf, se, sv


def band_conditions(g, band, band_surf, say=print):
    """The conditions on the fixture (tools/make_solar_audit_golden.py asserts them too): per set (weight set x sample count) the samples inside the band
    are at most 2 % and the rays inside the surface band at most 5 %; on each sharp set both classes hold at least 5 % of the samples."""
    R = int(g["lattice"][0]) * int(g["lattice"][1])
    for tag in TAGS:
        for S in S_LIST:
            n = nb = r = rb = sun = 0
            for vi in range(len(VIEWS)):
                for si in range(len(SUN_EL_AZ)):
                    conf, n_band, n_surf, _, _ = reference_of(g, key_of(tag, S, vi, si), band, band_surf)
                    n, nb, sun = n + R * S, nb + n_band, sun + conf["All_Solar_Vis"]["TP"] + conf["All_Solar_Vis"]["FN"]
                    r, rb = r + R, rb + n_surf
            say(f"  {tag} S={S}: {nb / n * 100:.3f} % of samples inside the band of {band:.2e}; {rb / r * 100:.2f} % of rays inside the surface band of "
                f"{band_surf:.2e}; in the sun {sun / n * 100:.1f} % of samples")
            assert nb <= 0.02 * n, (tag, S, nb, n)
            assert rb <= 0.05 * r, (tag, S, rb, r)
            if tag.startswith("sharp"):
                assert 0.05 * n <= sun <= 0.95 * n, (tag, S, sun, n)


def test_arguments_are_refused_by_name(built):      # noqa: F811
    import season_nerf_amd as sn
    L = sn._lib.lib()
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 31) & ~31
    sun = (C.c_double * 3)(0.3, -0.2, 0.8)
    ps = C.addressof(sun)

    def refused(args, what):
        L.snerf_field_ray_surface(None, 8, 96, None, None, None, 0, None, None)      # another entry point's message in between
        assert L.snerf_field_solar_audit(*args) == -1, what      # SNERF_E_INVALID
        assert b"snerf_field_solar_audit" in L.snerf_last_error(), (what, L.snerf_last_error())

    good = [None, 8, 96, p, p, p, ps, p, p, 2, p, None, None]      # only the model is missing
    refused(good, "NULL model")
    for k in (3, 4, 5, 6, 7, 8, 10):      # each required pointer NULL in turn (d_exact may be NULL)
        a = list(good)
        a[k] = None
        refused(a, f"argument {k} NULL")
    for k, v, what in ((1, -1, "n_rays < 0"), (2, 0, "n_samples < 1"), (10, p + 16, "d_out off 32 bytes"), (10, p + 4, "d_out off 32 bytes"),
                       (9, 1, "flags bit0"), (9, 8, "flags bit3"), (9, 16, "flags bit4")):
        a = list(good)
        a[k] = v
        refused(a, what)
    for bad in ((0.3, -0.2, 0.0), (0.3, -0.2, -0.8), (float("nan"), 0.0, 0.8), (0.3, float("inf"), 0.8), (0.3, 0.2, float("nan")), (0.3, 0.2, 1e-60)):
        s = (C.c_double * 3)(*bad)
        a = list(good)
        a[6] = C.addressof(s)
        refused(a, f"sun {bad}")
        assert b"sun" in L.snerf_last_error()
    # the last refusal of the list - a model whose resolved precision is not bf16x3 - needs a finalized model, i.e. a device: tests/test_gpu_audit.py::test_op


def test_kernels_are_in_the_code_objects_without_scratch(built):      # noqa: F811
    kernels = {}
    for elf in _device_code_objects(built.LIB):
        for k in _kernel_metadata(elf):
            kernels[k[".name"]] = k
    mine = {n: k for n, k in kernels.items() if "solar_audit_kernelI" in n or "solar_audit_ks_kernelI" in n}
    assert sorted(n.split("solar_audit_")[1].split("EEE")[0] for n in mine) == ["kernelILi256", "kernelILi64", "ks_kernelILi512"], sorted(mine)
    for n, k in mine.items():
        print(f"  {n}: vgpr {k['.vgpr_count']} agpr {k.get('.agpr_count')} sgpr {k['.sgpr_count']} spill {k['.vgpr_spill_count']} lds {k['.group_segment_fixed_size']}")
        assert k[".private_segment_fixed_size"] == 0, (n, "uses scratch")
        assert k[".max_flat_workgroup_size"] == 256, n


def test_ops_register_without_a_gpu(built):      # noqa: F811
    import season_nerf_amd as sn
    ns = sn.ops.load()
    assert hasattr(ns, "solar_audit")
    assert "float[] sun" in str(torch.ops.season_nerf.solar_audit.default._schema)
    for name in ("SolarAudit", "solar_audit", "audit_by_dir", "eval_solar_data", "advanced_solar"):
        assert hasattr(sn, name), name


def _view_rays(g, vi):
    """The ray grid of component_render_by_dir (mg_Img_Eval.py:99-104) for view vi of the fixture -> top, bot float32 [R,3]."""
    from season_nerf_amd.render import world_angle_2_local_vec
    H, Wd = (int(x) for x in g["lattice"])
    v = world_angle_2_local_vec(VIEWS[vi][0], VIEWS[vi][1], g["W2C"], g["W2L_H"])
    v = v / v[2]
    X, Y = np.meshgrid(np.linspace(1, -1, H), np.linspace(-1, 1, Wd), indexing="ij")
    grid = np.stack([X.ravel(), Y.ravel(), np.zeros(H * Wd)], 1)
    f = lambda a: torch.tensor(a, dtype=torch.float32)
    return f(grid + v.reshape(1, 3)), f(grid - v.reshape(1, 3))


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_meets_the_cpu_oracle(golden_dir, tag):
    """Fixture and tolerance fit each other before any GPU is involved.  The exact-solar block (mg_Img_Eval.py:57-70) restated on the CPU oracle's fp32
    network: the primary samples, the secondary rays Top = p + (1 - p_z) / sun_z * sun (float64 product and sum, cast to fp32), Bot = p, S samples,
    deltas zeroed outside the cube, exp(-sum of all but the last sample's rho delta) - in the band of the other fixture-vs-oracle tests.  The renders recorded per sample at S = 40
    keep it quick; the density forward is the whole cost."""
    g = fixture(golden_dir)
    sd = weights(golden_dir, tag)
    S = 40
    for vi, si in sorted((v, s_) for t_, S_, v, s_ in ARRAYS if t_ == tag and S_ == S):
        k = key_of(tag, S, vi, si)
        top, bot = _view_rays(g, vi)
        R = top.shape[0]
        pts, deltas = orc.sample_pt_coarse(top, bot, S, eval_mode=True, include_end_pt=True)
        deltas[orc.outside_cube(pts)] = 0.0
        np.testing.assert_allclose(deltas.reshape(R, S).numpy(), g[k + "_Deltas"], rtol=1e-6, atol=0)
        sun64 = g["sun_vecs"][si]
        sun32 = torch.tensor(sun64, dtype=torch.float32)
        p = pts.reshape(-1, 3)
        K = (1.0 - p[:, 2]) / sun32[2]
        top2 = (p.double() + K.double().unsqueeze(1) * torch.tensor(sun64).reshape(1, 3)).float()
        pts2, deltas2 = orc.sample_pt_coarse(top2, p, S, eval_mode=True, include_end_pt=True)
        deltas2[orc.outside_cube(pts2)] = 0.0
        with torch.no_grad():
            rho2 = orc.forward_sigma_only(sd, pts2.reshape(-1, 3)).reshape(R * S, S)
            rho = orc.forward_sigma_only(sd, p).reshape(R, S)
        exact = torch.exp(-(rho2 * deltas2.reshape(R * S, S))[:, :-1].sum(1)).reshape(R, S)
        np.testing.assert_allclose(exact.numpy(), g[k + "_Exact_Solar"], rtol=1e-4, atol=3e-5)
        np.testing.assert_allclose(rho.numpy(), g[k + "_Rho"], rtol=1e-4, atol=3e-5)


def test_mirrors_reproduce_the_reference(golden_dir):
    """`eval_solar_data` on the recorded arrays gives the recorded confusion dicts exactly; so does `SolarAudit.confusion()` on float64 sums of them (on
    the renders without per-sample arrays: of the recorded per-ray sums, for the surface counts); `_get_stats` gives the recorded statistics of every
    render to rtol 1e-12, NaN where the reference has NaN."""
    from season_nerf_amd.solar_audit import SolarAudit, _get_stats, _sums_f64, eval_solar_data
    g = fixture(golden_dir)
    n_nan = n_arrays = 0
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    for tag, S, vi, si, k in renders():
        rec = recorded_confusion(g, k)
        if (tag, S, vi, si) in ARRAYS:
            ex, es = g[k + "_Exact_Solar"].astype(np.float64), g[k + "_Est_Solar_Vis"].astype(np.float64)
            rho, dl = g[k + "_Rho"].astype(np.float64), g[k + "_Deltas"].astype(np.float64)
            got = eval_solar_data({"Exact_Solar": ex[..., None], "Est_Solar_Vis": es[..., None], "Rho": rho[..., None], "Deltas": dl[..., None]})
            assert got == rec, (k, got, rec)
            assert confusion_of_arrays(ex, es, ps_of(rho, dl)) == rec, k
            audit = SolarAudit(_sums_f64(t(ex), t(es), t(ps_of(rho, dl)))[None], S)
            assert audit.confusion(0) == rec and audit.confusion() == rec, (k, audit.confusion(0), rec)
            n_arrays += 1
        else:
            R = g[k + "_surf"].shape[1]
            sums = torch.zeros(1, R, 8, dtype=torch.float64)
            sums[0, :, 3], sums[0, :, 4] = t(g[k + "_surf"][0]), t(g[k + "_surf"][1])
            assert SolarAudit(sums, S).confusion(0)["Surface_Solar_Vis"] == rec["Surface_Solar_Vis"], k
        assert sum(rec["All_Solar_Vis"].values()) == int(g["lattice"][0]) * int(g["lattice"][1]) * S
        for i, fam in enumerate(FAMILIES):
            stats = _get_stats(*(rec[fam][c] for c in CONF_KEYS))
            np.testing.assert_allclose(np.array(stats, dtype=np.float64), g[k + "_stats"][i], rtol=1e-12, atol=0, equal_nan=True, err_msg=f"{k} {fam}")
            n_nan += int(np.isnan(g[k + "_stats"][i]).sum())
    assert n_arrays == len(ARRAYS)
    print(f"  renders with per-sample arrays: {n_arrays}; recorded statistics that are NaN: {n_nan}")


def test_shadow_analyasis_and_nan_cases(golden_dir):
    """`_shadow_analyasis` on a region built from the recorded counts: the per-cell statistics are `_get_stats` of the cells (the recorded ones), "Overall"
    those of the summed counts; an empty class gives NaN where numpy's division gives the reference NaN."""
    from season_nerf_amd.solar_audit import _BASE_KEYS, _get_stats, _shadow_analyasis
    g = fixture(golden_dir)
    tag, S = "sharp_W64", 40
    shape = (len(VIEWS), len(SUN_EL_AZ))
    region = {fam: {c: np.zeros(shape) for c in CONF_KEYS} for fam in FAMILIES}
    for vi in range(shape[0]):
        for si in range(shape[1]):
            for i, fam in enumerate(FAMILIES):
                for j, c in enumerate(CONF_KEYS):
                    region[fam][c][vi, si] = g[key_of(tag, S, vi, si) + "_confusion"][i, j]
    out = _shadow_analyasis({"A": region})
    assert out["A"] is region
    for i, fam in enumerate(FAMILIES):
        for n, name in enumerate(_BASE_KEYS):
            for vi in range(shape[0]):
                for si in range(shape[1]):
                    np.testing.assert_allclose(region[fam][name][vi, si], g[key_of(tag, S, vi, si) + "_stats"][i, n], rtol=1e-12, atol=0, equal_nan=True)
        overall = _get_stats(*(region[fam][c].sum() for c in CONF_KEYS))
        for n, name in enumerate(_BASE_KEYS):
            np.testing.assert_allclose(region[fam]["Overall"][name], overall[n], rtol=1e-12, atol=0, equal_nan=True)
    acc, bal, prev, pp, rp, pn, rn, f1p, f1n = _get_stats(0, 10, 0, 0)      # nothing in the sun
    assert acc == 1.0 and prev == 1.0 and pn == 1.0 and rn == 1.0 and f1n == 1.0 and all(np.isnan(x) for x in (bal, pp, rp, f1p))
    assert all(np.isnan(x) for x in _get_stats(0, 0, 0, 0))
    arr = _get_stats(np.array([3, 0]), np.array([5, 4]), np.array([1, 0]), np.array([1, 0]))
    assert arr[0].shape == (2,) and arr[0][0] == 0.8 and np.isnan(arr[3][1]) and not np.isnan(arr[3][0])


def test_band_conditions(golden_dir):
    """Conditions on the fixture, not measurements: a band that breaks them would make the count comparison of the GPU test say little."""
    g = fixture(golden_dir)
    assert BAND > 0 and BAND == 2 * max(E_EXACT, E_EST) and BAND_SURF == 2 * E_SURF
    band_conditions(g, BAND, BAND_SURF)
