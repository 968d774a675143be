"""CPU-only checks of the shadow-walk feature (the reference's shadow test scored inside the field kernel): the C ABI's argument check, the three
kernels in the shipped code objects, `ShadowWalk.scores` against the reference's recorded scores, the `shadow_points.npz` fixture against the CPU
oracle, and the conditions the comparison band of tests/test_gpu_shadow.py has to meet on that fixture.

The band.  Measured on an MI355X with the per-sample path the feature does not touch (`T_NeRF.forward_Solar` + `get_PV` on the fixture's rays, i.e.
`eval_shadow_data`), over the whole fixture (4 weight sets x 2 sample counts x 5 suns x 36 ground points), printed by
    python -m pytest tests/test_gpu_shadow.py -m gpu -k per_sample_deviation -s
E_VIS = max |vis - Est_Vis_ref|, E_PV = max |PV - Exact_Vis_ref|.  BAND = 2 max(E_VIS, E_PV): a reference sample whose exact or learned visibility lies
within BAND of .5 may be counted on either side by the device; the factor 2 covers the kernel's different summation order in the prefix."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc
from test_isa_guards import _device_code_objects, _kernel_metadata
from test_surface_host import TAGS, built, weights      # noqa: F401  (built: the session fixture)

E_VIS = 3.43e-5      # measured 3.4213e-05 (sharp_W64, Z = 40), rounded up
E_PV = 2.04e-4       # measured 2.0355e-04 (sharp_W64, Z = 40), rounded up; the reference's own fp32 error against float64 there: 6.5e-5
BAND = 2 * max(E_VIS, E_PV)
KEYS = ("Acc", "Prec_Sun", "Recall_Sun", "Prec_Shadow", "Recall_Shadow", "Loss", "Avg_Error", "Avg_Offset")


def fixture(golden_dir):
    g = dict(np.load(os.path.join(golden_dir, "shadow_points.npz"), allow_pickle=False))
    assert list(g["tags"]) == TAGS and list(g["score_keys"]) == list(KEYS)
    return g


def fixture_rays(g):
    """The rays of the fixture as eval_shadow_data lays them (mg_Shadow_Eval.py:80-83): ground -+ sun_vec / sun_vec_z in float64, cast to float32.
    -> top, bot, sun [M G, 3] float32 (sun: the unit vector of world_angle_2_local_vec, repeated per ground point)."""
    orig = g["sun_vecs"]
    step = orig / orig[:, 2:3]
    G = g["ground_points"].shape[0]
    g3 = np.zeros([1, G, 3])
    g3[0, :, :2] = g["ground_points"]
    f = lambda a: torch.tensor(a, dtype=torch.float32).reshape(-1, 3)
    return f(g3 + step[:, None, :]), f(g3 - step[:, None, :]), f(np.repeat(orig[:, None, :], G, 1))


def eight_sums(pv, vis, y):
    """The eight per-ray sums of snerf_field_shadow_walk from per-sample PV, vis and y = rho delta [R,S], in their dtype."""
    ps = pv * (1 - torch.exp(-y))
    ex, es = pv > 0.5, vis > 0.5
    d = pv - vis
    cnt = lambda m: m.sum(1).to(pv.dtype)
    return torch.stack([cnt(ex & es), cnt(ex), cnt(es), (d * d).sum(1), d.abs().sum(1), (ps * vis).sum(1), ps.sum(1), y.sum(1)], 1)


def sums_of_arrays(exact, est):
    """[M,G,Z] per-sample arrays -> [M G, 8] float64 rows with the five slots the scores read (the others zero)."""
    pv, vis = torch.tensor(exact, dtype=torch.float64).reshape(-1, exact.shape[-1]), torch.tensor(est, dtype=torch.float64).reshape(-1, exact.shape[-1])
    return eight_sums(pv, vis, torch.zeros_like(pv))


def in_band(exact, est, band):
    """Samples of the reference whose exact or learned visibility lies within `band` of .5 -> bool, the arrays' shape."""
    return (np.abs(exact.astype(np.float64) - .5) <= band) | (np.abs(est.astype(np.float64) - .5) <= band)


REF_ERR = {}


def reference_error(golden_dir, g, tag, Z):
    """The reference's own error on a set of the fixture: max |its fp32 arrays - the CPU oracle in float64 on the same fp32 rays and weights|
    -> (for Exact_Vis, for Est_Vis); computed once per set."""
    if (tag, Z) not in REF_ERR:
        sd = {k: (v.double() if v.is_floating_point() else v) for k, v in weights(golden_dir, tag).items()}
        top, bot, sun = fixture_rays(g)
        R = top.shape[0]
        pts, deltas = orc.sample_pt_coarse(top, bot, Z, eval_mode=True)
        deltas[orc.outside_cube(pts)] = 0.0
        with torch.no_grad():
            rho, vis, _ = orc.forward_solar(sd, pts.reshape(-1, 3).double(), sun.unsqueeze(1).expand(R, Z, 3).reshape(-1, 3).double())
        pv = orc.get_PV(rho.reshape(R, Z, 1), deltas.double())
        shape = g[f"{tag}_Z{Z}_Exact_Vis"].shape
        REF_ERR[(tag, Z)] = (float(np.abs(pv.reshape(shape).numpy() - g[f"{tag}_Z{Z}_Exact_Vis"]).max()),
                             float(np.abs(vis.reshape(shape).numpy() - g[f"{tag}_Z{Z}_Est_Vis"]).max()))
    return REF_ERR[(tag, Z)]


def test_arguments_are_refused_by_name(built):      # noqa: F811
    import season_nerf_amd as sn
    L = sn._lib.lib()
    assert L.snerf_field_shadow_walk(None, 8, 96, None, None, None, None, 0, None, None) == -1      # SNERF_E_INVALID
    assert b"snerf_field_shadow_walk" in L.snerf_last_error()
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 31) & ~31
    for n_rays, n_samples, out in ((8, 0, p), (-1, 96, p), (8, 96, p + 16), (8, 96, p + 4)):
        L.snerf_field_ray_surface(None, 8, 96, None, None, None, 0, None, None)      # another entry point's message in between
        assert L.snerf_field_shadow_walk(None, n_rays, n_samples, p, p, p, p, 0, out, None) == -1, (n_rays, n_samples, out - p)
        assert b"snerf_field_shadow_walk" in L.snerf_last_error(), (n_rays, n_samples, out - p)
    for k in range(4):      # each of the four inputs NULL in turn
        a = [p] * 4
        a[k] = None
        assert L.snerf_field_shadow_walk(None, 8, 96, *a, 0, p, None) == -1 and b"snerf_field_shadow_walk" in L.snerf_last_error()


def test_kernels_are_in_the_code_objects_without_scratch(built):      # noqa: F811
    kernels = {}
    for elf in _device_code_objects(built.LIB):
        for k in _kernel_metadata(elf):
            kernels[k[".name"]] = k
    mine = {n: k for n, k in kernels.items() if "shadow_walk_kernelI" in n or "shadow_walk_ks_kernelI" in n}
    assert sorted(n.split("shadow_walk_")[1].split("EEE")[0] for n in mine) == ["kernelILi256", "kernelILi64", "ks_kernelILi512"], sorted(mine)
    for n, k in mine.items():
        print(f"  {n}: vgpr {k['.vgpr_count']} agpr {k.get('.agpr_count')} sgpr {k['.sgpr_count']} spill {k['.vgpr_spill_count']} lds {k['.group_segment_fixed_size']}")
        assert k[".private_segment_fixed_size"] == 0, (n, "uses scratch")
        assert k[".max_flat_workgroup_size"] == 256, n


@pytest.mark.parametrize("Z", [96, 40])
@pytest.mark.parametrize("tag", TAGS)
def test_scores_reproduce_the_reference(golden_dir, tag, Z):
    """Per-ray sums formed in float64 from the reference's per-sample arrays -> the reference's own scores; the mirror of shadow_anaylysis likewise."""
    from season_nerf_amd.shadow_eval import ShadowWalk, shadow_anaylysis
    g = fixture(golden_dir)
    exact, est, ref = g[f"{tag}_Z{Z}_Exact_Vis"], g[f"{tag}_Z{Z}_Est_Vis"], g[f"{tag}_Z{Z}_scores"]
    M, G = exact.shape[:2]
    sw = ShadowWalk(sums_of_arrays(exact, est), Z)
    got = sw.scores()
    mir = shadow_anaylysis(g["ground_points"], g["shadow_angles"], {"Exact_Vis": exact.astype(np.float64)[..., None], "Est_Vis": est.astype(np.float64)[..., None]})
    for i, k in enumerate(KEYS):
        print(f"  {tag} Z={Z} {k:14s} {got[k]:.15g} (reference {ref[i]:.15g})")
        np.testing.assert_allclose(got[k], ref[i], rtol=1e-12, atol=0, equal_nan=True, err_msg=k)
        np.testing.assert_allclose(mir[k], ref[i], rtol=1e-12, atol=0, equal_nan=True, err_msg="mirror " + k)
    # one sun at a time: the mask, and per_sun's layout
    ps = sw.per_sun(M, G)
    assert ps.sums.shape == (M, G, 8) and torch.equal(ps.n_exact[2], sw.n_exact[2 * G:3 * G])
    for m in range(M):
        mask = torch.zeros(M, G, dtype=torch.bool)
        mask[m] = True
        one = shadow_anaylysis(None, None, {"Exact_Vis": exact[m:m + 1].astype(np.float64), "Est_Vis": est[m:m + 1].astype(np.float64)})
        got_m = sw.scores(mask)
        for k in KEYS:
            np.testing.assert_allclose(got_m[k], one[k], rtol=1e-12, atol=0, equal_nan=True, err_msg=f"sun {m} {k}")


def test_empty_class_gives_nan():
    """What numpy's division gives the reference: no sample in the sun -> Prec_Sun and Recall_Sun are 0 / 0; everything in the sun -> the shadow's."""
    from season_nerf_amd.shadow_eval import ShadowWalk, shadow_anaylysis
    R, S = 6, 17
    for fill, nan_keys in ((0.1, ("Prec_Sun", "Recall_Sun")), (0.9, ("Prec_Shadow", "Recall_Shadow"))):
        a = np.full([1, R, S], fill)
        got = ShadowWalk(sums_of_arrays(a, a), S).scores()
        with np.errstate(invalid="ignore", divide="ignore"):
            ref = shadow_anaylysis(None, None, {"Exact_Vis": a[..., None], "Est_Vis": a[..., None]})
        for k in KEYS:
            assert np.isnan(got[k]) == (k in nan_keys) and np.isnan(ref[k]) == (k in nan_keys), (fill, k, got[k], ref[k])
        assert got["Acc"] == 1.0 and got["Loss"] == 0.0 and got["Avg_Offset"] == 0.0
    none = ShadowWalk(torch.zeros(0, 8, dtype=torch.float64), S).scores()
    assert all(np.isnan(none[k]) for k in KEYS)


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_meets_the_cpu_oracle(golden_dir, tag):
    """Fixture and tolerance fit each other before any GPU is involved: the oracle's fp32 network on the fixture's rays (the band of the other
    fixture-vs-oracle tests)."""
    g = fixture(golden_dir)
    sd = weights(golden_dir, tag)
    top, bot, sun = fixture_rays(g)
    R = top.shape[0]
    for Z in (int(z) for z in g["Z_list"]):
        pts, deltas = orc.sample_pt_coarse(top, bot, Z, eval_mode=True)
        deltas[orc.outside_cube(pts)] = 0.0
        with torch.no_grad():
            rho, vis, sky = orc.forward_solar(sd, pts.reshape(-1, 3), sun.unsqueeze(1).expand(R, Z, 3).reshape(-1, 3))
        pv = orc.get_PV(rho.reshape(R, Z, 1), deltas)
        shape = g[f"{tag}_Z{Z}_Exact_Vis"].shape
        np.testing.assert_allclose(pv.reshape(shape).numpy(), g[f"{tag}_Z{Z}_Exact_Vis"], rtol=1e-4, atol=3e-5)
        np.testing.assert_allclose(vis.reshape(shape).numpy(), g[f"{tag}_Z{Z}_Est_Vis"], rtol=1e-4, atol=3e-5)
        np.testing.assert_allclose(sky.reshape(shape[0], -1, 3)[:, 0].numpy(), g[f"{tag}_Z{Z}_Sky_Col"], rtol=1e-4, atol=1e-4)


def test_band_conditions(golden_dir):
    """With the measured band: the samples inside it are at most 2 % of each set's samples, and on the three sharp sets at least half of the rays have
    none.  (Conditions on the fixture, not measurements: a band that breaks them would make the count comparison of the GPU test say little.)"""
    g = fixture(golden_dir)
    assert BAND > 0 and BAND == 2 * max(E_VIS, E_PV)
    for tag in TAGS:
        for Z in (int(z) for z in g["Z_list"]):
            b = in_band(g[f"{tag}_Z{Z}_Exact_Vis"], g[f"{tag}_Z{Z}_Est_Vis"], BAND)
            share, free = b.mean(), 1.0 - b.any(2).mean()
            print(f"  {tag} Z={Z}: {share * 100:.3f} % of samples inside the band of {BAND:.2e}; {free * 100:.1f} % of rays have none")
            assert share <= 0.02, (tag, Z, share)
            if tag.startswith("sharp"):
                assert free >= 0.5, (tag, Z, free)
