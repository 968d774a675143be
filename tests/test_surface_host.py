"""CPU-only checks of the ray-surface feature (height maps from a density-only ray pass): the C ABI's argument check, the three kernels in the
shipped code objects, `RaySurface`'s formulas against the oracle's, and the `height_columns.npz` fixture against the CPU oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc
from test_isa_guards import _device_code_objects, _kernel_metadata

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD = ("G_NeRF_net.fc10Sigma.weight", "G_NeRF_net.fc10Sigma.bias")
TAGS = ["init_W64_s2", "sharp_W64", "sharp_W256", "sharp_W512"]


@pytest.fixture(scope="session")
def built():
    import importlib.util
    spec = importlib.util.spec_from_file_location("snerf_build", os.path.join(REPO, "season_nerf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    b.build_ops()
    return b


def weights(golden_dir, tag):
    """The state dict of a weight set of height_columns.npz: the init law, or a trained fixture with the density head scaled by the g of sharp_W*.npz
    (as `sharp_net` of test_gpu_render.py builds it)."""
    if tag == "init_W64_s2":
        return orc.init_weights(64, 4, 2)
    g = dict(np.load(os.path.join(golden_dir, tag + ".npz"), allow_pickle=False))
    t = dict(np.load(os.path.join(golden_dir, str(g["source"])), allow_pickle=False))
    return {k[3:]: torch.tensor(v) * (float(g["g"]) if k[3:] in HEAD else 1.0) for k, v in t.items() if k.startswith("sd_")}


def lattice(shape):
    """eval_HM's columns as rays (Eval_funcs.py:299-312): top z = +1, bot z = -1 at x = 2 i / H - 1, y = 2 j / W - 1 -> (top, bot) float32 [H W, 3]."""
    H, W = int(shape[0]), int(shape[1])
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xy = np.stack([ii.reshape(-1) * (1.0 / H) * 2 - 1, jj.reshape(-1) * (1.0 / W) * 2 - 1], 1)
    f = lambda z: torch.tensor(np.concatenate([xy, np.full([H * W, 1], z)], 1), dtype=torch.float32)
    return f(1.0), f(-1.0)


def oracle_density(sd, top, bot, tv):
    """fp32 density of the CPU oracle at the samples of the rays -> [R, S] (points as misc.py:240-241 forms them)."""
    t = tv.reshape(1, -1, 1)
    pts = top.unsqueeze(1) * (1 - t) + bot.unsqueeze(1) * t
    with torch.no_grad():
        return orc.forward_sigma_only(sd, pts.reshape(-1, 3)).reshape(top.shape[0], tv.numel())


def four_sums(rho, delta, tv):
    """{sum PS, sum PS t, sum PS s, optical depth} of rays in the dtype of the arguments (rho, delta [R,S]; tv [S]); PV as get_PV forms it."""
    y = rho * delta
    c = torch.cumsum(torch.cat([torch.zeros_like(y[:, :1]), y], 1), 1)
    ps = torch.exp(-c[:, :-1]) * (1 - torch.exp(-y))
    idx = torch.arange(rho.shape[1], dtype=rho.dtype, device=rho.device)
    return ps.sum(1), (ps * tv.to(rho.dtype).reshape(1, -1)).sum(1), (ps * idx).sum(1), c[:, -1]


def test_null_pointers_are_refused_by_name(built):
    import season_nerf_amd as sn
    L = sn._lib.lib()
    assert L.snerf_field_ray_surface(None, 8, 96, None, None, None, 0, None, None) == -1      # SNERF_E_INVALID
    assert b"snerf_field_ray_surface" in L.snerf_last_error()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert L.snerf_field_ray_surface(None, 8, 0, p, p, p, 0, p, None) == -1 and b"snerf_field_ray_surface" in L.snerf_last_error()
    assert L.snerf_field_ray_surface(None, -1, 96, p, p, p, 0, p, None) == -1 and b"snerf_field_ray_surface" in L.snerf_last_error()


def test_kernels_are_in_the_code_objects_without_scratch(built):
    kernels = {}
    for elf in _device_code_objects(built.LIB):
        for k in _kernel_metadata(elf):
            kernels[k[".name"]] = k
    mine = {n: k for n, k in kernels.items() if "ray_surface_kernelI" in n or "ray_surface_ks_kernelI" in n}
    assert sorted(n.split("ray_surface_")[1].split("EEE")[0] for n in mine) == ["kernelILi256", "kernelILi64", "ks_kernelILi512"], sorted(mine)
    for n, k in mine.items():
        print(f"  {n}: vgpr {k['.vgpr_count']} agpr {k.get('.agpr_count')} sgpr {k['.sgpr_count']} spill {k['.vgpr_spill_count']} lds {k['.group_segment_fixed_size']}")
        assert k[".private_segment_fixed_size"] == 0, (n, "uses scratch")
        assert k[".max_flat_workgroup_size"] == 256, n


def test_formulas_match_the_oracle():
    from season_nerf_amd.render import RaySurface
    rng = np.random.Generator(np.random.PCG64(5))
    for S in (1, 2, 33, 96):
        R = 17
        PS = torch.tensor(rng.uniform(0, 1, (R, S, 1)) ** 4 / S)
        top = torch.tensor(rng.uniform(-1, 1, (R, 3)))
        bot = torch.tensor(rng.uniform(-1, 1, (R, 3)))
        tv = torch.linspace(0, 1, S + 1, dtype=torch.float64)[:-1]
        t = tv.reshape(1, S, 1)
        pts = top.unsqueeze(1) * (1 - t) + bot.unsqueeze(1) * t
        delta = torch.sqrt(((top - bot) ** 2).sum(1)) / S
        deltas = delta.reshape(R, 1, 1).expand(R, S, 1)
        idx = torch.arange(S, dtype=torch.float64).reshape(1, S, 1)
        rs = RaySurface(PS.sum(1)[:, 0], (PS * t).sum(1)[:, 0], (PS * idx).sum(1)[:, 0], torch.zeros(R, dtype=torch.float64), S, delta)
        loc, dist = orc.surface_depth(PS, pts, deltas)
        np.testing.assert_allclose(rs.surface_location(top, bot).numpy(), loc.numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(rs.surface_distance().numpy(), dist[:, 0].numpy(), rtol=1e-12, atol=1e-12)
        dsm = (PS.numpy() * np.linspace(1, -1, S).reshape(1, -1, 1)).sum(1)[:, 0]      # the sum of quick_run_dsm (Quick_Run.py:39)
        np.testing.assert_allclose(rs.dsm().numpy(), dsm, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(rs.expected_height().numpy(), dsm / PS.sum(1)[:, 0].numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(rs.opacity().numpy(), PS.sum(1)[:, 0].numpy(), rtol=0, atol=0)
        assert torch.equal(rs.transmittance(), torch.ones(R, dtype=torch.float64))


@pytest.mark.parametrize("tag", TAGS)
def test_fixture_meets_the_cpu_oracle(golden_dir, tag):
    """Fixture and tolerance fit each other before any GPU is involved: the oracle's fp32 density on the lattice, the formulas in float64."""
    from season_nerf_amd.render import RaySurface
    g = dict(np.load(os.path.join(golden_dir, "height_columns.npz"), allow_pickle=False))
    assert list(g["tags"]) == TAGS
    H, W, n = (int(v) for v in g["shape"])
    top, bot = lattice((H, W))
    tv = torch.linspace(0, 1, n + 1)[:-1].float()
    rho = oracle_density(weights(golden_dir, tag), top, bot, tv).double()
    acc, mt, mi, carry = four_sums(rho, torch.full_like(rho, 2.0 / n), tv)
    rs = RaySurface(acc, mt, mi, carry, n, torch.full([H * W], 2.0 / n, dtype=torch.float64))
    np.testing.assert_allclose(rs.opacity().reshape(H, W).numpy(), g[tag + "_P_Surf_sum"], rtol=1e-4, atol=3e-5)
    np.testing.assert_allclose(rs.expected_height().reshape(H, W).numpy(), g[tag + "_Est_HM"], rtol=1e-4, atol=3e-5)
