"""The sun walk on the GPU: M sun directions (and M x T sun / season images) of one view from one pass of the field network
(`component_render_sun_walk`, `render_sun_season_walk`, csrc/kernels.hip sun_walk_kernel / sun_walk_composite_kernel, csrc/kernels_ks.hip
sun_walk_ks_kernel) against the reference's own per-sun renders, against this package's single-sun path bit for bit, and against the oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-5)
DEV = torch.device("cuda")


def close(name, a, b, **kw):
    kw = {**TOL, **kw}
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    print(f"  {name:26s} max abs {np.abs(a - b).max():.3e}")
    np.testing.assert_allclose(a, b, err_msg=name, **kw)


def make_net(W, C=4, seed=2, precision="bf16x3"):
    import season_nerf_amd as sn
    net = sn.T_NeRF(W, C)
    net.load_state_dict(orc.init_weights(W, C, seed))
    if precision is not None:
        net.precision = precision
    return net.to("cuda").eval()


@pytest.fixture(scope="module")
def fx(golden_dir):
    import season_nerf_amd as sn
    g = dict(np.load(os.path.join(golden_dir, "sun_walk_W64.npz"), allow_pickle=False))
    net = make_net(int(g["W"]), int(g["C"]), int(g["seed"]))
    suns = [tuple(s) for s in g["suns"]]
    size = tuple(int(v) for v in g["size"])
    walk = sn.component_render_sun_walk(net, tuple(g["view"]), suns, float(g["times"][0]), size, g["WC"], g["H"], DEV)
    return sn, g, net, suns, size, walk


def test_walk_against_the_reference_fixture(fx):
    """W = 64, (6, 7, 40) = 1680 points = 13 tiles of 128 + 16 points: per-sun Est_Solar_Vis and Sky_Col and the M x T images against the reference's
    component_render_by_dir / get_imgs_from_Img_Dict_t_step per (sun, time), at the tolerance tests/test_gpu_render.py holds the same keys to."""
    sn, g, net, suns, size, walk = fx
    assert len(walk) == len(suns) == 5
    d0 = walk[0]
    close("Deltas", d0["Deltas"], g["Deltas"], rtol=1e-6, atol=0)
    close("Rho", d0["Rho"], g["Rho"], rtol=2e-4, atol=2e-5)
    close("Base_Col", d0["Base_Col"], g["Base_Col"], atol=1e-4)
    close("Adjust_col", d0["Adjust_col"], g["Adjust_col"], atol=1e-4)
    for j in range(len(suns)):
        close(f"Est_Solar_Vis[{j}]", walk[j]["Est_Solar_Vis"], g["Est_Solar_Vis"][j])
        close(f"Sky_Col[{j}]", walk[j]["Sky_Col"][0, 0], g["Sky_Col0"][j])
        # the dict of sun j through an existing consumer
        close(f"t_step[{j}]", sn.get_imgs_from_Img_Dict_t_step(walk[j], size, g["classes"]), g["imgs"][j])
    imgs, mask = sn.render_sun_season_walk(net, tuple(g["view"]), suns, [float(t) for t in g["times"]], size, g["WC"], g["H"], DEV)
    assert imgs.shape == (5, 3, 6, 7, 3) and imgs.dtype == torch.float32 and imgs.is_cuda and mask.shape == (5, 6, 7)
    close("imgs", imgs.cpu().numpy(), g["imgs"])
    for j in range(len(suns)):
        close(f"Shadow_Mask[{j}]", mask[j].cpu().numpy(), sn.get_imgs_from_Img_Dict(walk[j], size, False)["Shadow_Mask"])


SHARED = ["World_Points", "Rho", "Base_Col", "Adjust_col"]


def _single(sn, net, view, sun, tf, size, g):
    return sn.component_render_by_dir(net, view, sun, tf, size, g["WC"], g["H"], DEV, include_exact_solar=False)


def _assert_identical(walk, singles):
    for k in SHARED:
        assert torch.equal(walk.dev[k], singles[0].dev[k]), k
    for j, s in enumerate(singles):
        assert torch.equal(walk[j].dev["Est_Solar_Vis"], s.dev["Est_Solar_Vis"]), ("Est_Solar_Vis", j)
        assert torch.equal(walk[j].dev["Sky"], s.dev["Sky"]), ("Sky", j)
        assert np.array_equal(walk[j]["Est_Solar_Vis"], s["Est_Solar_Vis"]) and np.array_equal(walk[j]["Sky_Col"], s["Sky_Col"])


@pytest.mark.parametrize("W", [64, 256, 512])
def test_walk_is_bit_identical_to_the_single_sun_path(fx, W):
    """(24, 24, 64) = 36 864 points: 288 tiles of 128 / 576 tiles of 64, more than the 256 workgroups - some workgroups run a second tile and the ring
    wraps from the adjust chunks back to fc1.  The walk runs the same run_layer arithmetic on the same fragments: atol = rtol = 0, for M = 3 and M = 1."""
    sn, g = fx[0], fx[1]
    net = make_net(W, 4, 5)
    assert net.resolved_precision == "bf16x3"
    size, view, suns = (24, 24, 64), (65, 40), [(30, 90), (55, 210), (75, 330)]
    singles = [_single(sn, net, view, s, 0.3, size, g) for s in suns]
    walk = sn.component_render_sun_walk(net, view, suns, 0.3, size, g["WC"], g["H"], DEV)
    assert len(walk) == 3
    _assert_identical(walk, singles)
    one = sn.component_render_sun_walk(net, view, suns[1:2], 0.3, size, g["WC"], g["H"], DEV)
    assert len(one) == 1
    _assert_identical(one, singles[1:2])


def _grid_oracle(plain, sv_all, sky_all, size, cv):
    """orc.images_t_step per sun direction (float64)."""
    R, S = plain["Rho"].shape[:2]
    out = []
    for j in range(sv_all.shape[0]):
        d = dict(plain)
        d["Est_Solar_Vis"] = sv_all[j]
        d["Sky_Col"] = np.broadcast_to(sky_all[j].reshape(1, 1, 3), (R, S, 3))
        out.append(orc.images_t_step(d, size, cv))
    return np.stack(out)


def test_grid_compositing_kernel_vs_oracle(fx):
    """The compositing kernel on its own: M = 7 (several passes over the suns do not happen at 7, over the class vectors they do: T = 13 > 6 per pass),
    arbitrary class vectors, against the oracle's float64 get_imgs_from_Img_Dict_t_step per sun, at the tolerance of test_sweep_many_time_steps_vs_oracle;
    again from a plain dict with explicit Deltas; again with M = 9 > 8 per pass; again with M = T = 1."""
    sn, g, net, suns, size, walk = fx
    from season_nerf_amd import render as R_
    rng = np.random.Generator(np.random.PCG64(11))
    d = dict(walk.dev)
    sv5, sky5 = d["Solar_Vis_All"], d["Sky_All"]
    for M in (7, 9):
        idx = [j % 5 for j in range(M)]
        pert = torch.tensor(rng.uniform(0.0, 0.2, (M, 1, 1, 1)), dtype=torch.float32, device=DEV)
        sv = (sv5[idx] * (1.0 - pert) + pert * torch.tensor(rng.uniform(0, 1, tuple(sv5[idx].shape)), dtype=torch.float32, device=DEV)).contiguous()
        sky = torch.tensor(rng.uniform(0, 1, (M, 3)), dtype=torch.float32, device=DEV)
        d["Solar_Vis_All"], d["Sky_All"] = sv, sky
        cv = rng.uniform(-0.5, 1.5, (13, 4))
        o = R_._composite_sun_walk(d, cv)
        plain = {k: np.asarray(v) for k, v in walk[0].items()}
        ref = _grid_oracle(plain, sv.cpu().numpy().astype(np.float64), sky.cpu().numpy().astype(np.float64), size, cv)
        got = o["shaded"].cpu().numpy().reshape(M, 13, size[0], size[1], 3)
        assert got.shape == ref.shape
        close(f"grid M={M}", got, ref, rtol=1e-5, atol=1e-6)
        # season and shadow_adjust multiply to shaded; raw_shadow is the sweep kernel's
        close("season x shadow_adjust", (o["season"][None] * o["shadow_adjust"][:, None]).cpu().numpy(), o["shaded"].cpu().numpy(), rtol=1e-6, atol=1e-7)
        d1 = dict(d, Est_Solar_Vis=sv[3].contiguous(), Sky=sky[3].contiguous())
        sw = R_._sweep(d1, cv, "Est_Solar_Vis")
        close("raw_shadow", o["raw_shadow"][3].cpu().numpy(), sw["raw_shadow"].cpu().numpy(), rtol=1e-5, atol=1e-6)
        close("base", o["base"].cpu().numpy(), sw["base"].cpu().numpy(), rtol=1e-5, atol=1e-6)
        # a plain dict carrying explicit Deltas (no top / bot / tvals)
        f = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.float32)), device=DEV)
        dp = {"Rho": f(plain["Rho"]), "Deltas_explicit": f(plain["Deltas"]), "Base_Col": f(plain["Base_Col"]), "Adjust_col": f(plain["Adjust_col"]),
              "Solar_Vis_All": sv, "Sky_All": sky}
        got2 = R_._composite_sun_walk(dp, cv)["shaded"].cpu().numpy().reshape(ref.shape)
        close(f"grid M={M} explicit deltas", got2, ref, rtol=1e-5, atol=1e-6)
    d["Solar_Vis_All"], d["Sky_All"] = sv[:1].contiguous(), sky[:1].contiguous()
    got1 = R_._composite_sun_walk(d, cv[4:5])["shaded"].cpu().numpy().reshape(1, 1, size[0], size[1], 3)
    close("grid M=T=1", got1, ref[:1, 4:5], rtol=1e-5, atol=1e-6)


def test_ray_blocks_equal_the_full_grid(fx):
    """ray_range blocks of parallel.shard_bounds(H * W, 3) concatenated along the ray axis are the full result, bit for bit; so are the walk's own ray
    blocks (the launches of a walk whose solar_vis would pass the size cap)."""
    sn, g, net, suns, size, walk = fx
    from season_nerf_amd import render as R_
    times = [float(t) for t in g["times"]]
    args = (net, tuple(g["view"]), suns, times, size, g["WC"], g["H"], DEV)
    imgs, mask = sn.render_sun_season_walk(*args)
    parts = [sn.render_sun_season_walk(*args, ray_range=b) for b in sn.parallel.shard_bounds(size[0] * size[1], 3)]
    assert torch.equal(torch.cat([p[0] for p in parts], 2), imgs.reshape(5, 3, -1, 3))
    assert torch.equal(torch.cat([p[1] for p in parts], 1), mask.reshape(5, -1))
    cap = R_.WALK_SOLAR_VIS_BYTES
    try:
        R_.WALK_SOLAR_VIS_BYTES = 4 * 40 * 5 * 11          # 11 rays per launch: 42 rays in four blocks
        blocked = sn.component_render_sun_walk(net, tuple(g["view"]), suns, times[0], size, g["WC"], g["H"], DEV)
    finally:
        R_.WALK_SOLAR_VIS_BYTES = cap
    for k in SHARED + ["Solar_Vis_All", "Sky_All", "Deltas"]:
        assert torch.equal(blocked.dev[k], walk.dev[k]), k


def test_more_than_32_suns(fx):
    """M = 35 at (4, 4, 24): two walk launches (32 + 3 sun directions), equal to the walks of the two batches and to the single-sun path."""
    sn, g, net = fx[0], fx[1], fx[2]
    size, view = (4, 4, 24), (70, 20)
    suns = [(20.0 + 2.0 * j, (37.0 * j) % 360.0) for j in range(35)]
    walk = sn.component_render_sun_walk(net, view, suns, 0.45, size, g["WC"], g["H"], DEV)
    assert len(walk) == 35
    a = sn.component_render_sun_walk(net, view, suns[:32], 0.45, size, g["WC"], g["H"], DEV)
    b = sn.component_render_sun_walk(net, view, suns[32:], 0.45, size, g["WC"], g["H"], DEV)
    assert torch.equal(walk.dev["Solar_Vis_All"], torch.cat([a.dev["Solar_Vis_All"], b.dev["Solar_Vis_All"]], 0))
    assert torch.equal(walk.dev["Sky_All"], torch.cat([a.dev["Sky_All"], b.dev["Sky_All"]], 0))
    for k in SHARED:
        assert torch.equal(walk.dev[k], a.dev[k]) and torch.equal(walk.dev[k], b.dev[k]), k
    picks = [0, 31, 32, 34]
    singles = [_single(sn, net, view, suns[j], 0.45, size, g) for j in picks]
    for k in SHARED:
        assert torch.equal(walk.dev[k], singles[0].dev[k]), k
    for j, s in zip(picks, singles):
        assert torch.equal(walk[j].dev["Est_Solar_Vis"], s.dev["Est_Solar_Vis"]) and torch.equal(walk[j].dev["Sky"], s.dev["Sky"]), j
    imgs, mask = sn.render_sun_season_walk(net, view, suns, [0.2, 0.7], size, g["WC"], g["H"], DEV)
    assert imgs.shape == (35, 2, 4, 4, 3) and mask.shape == (35, 4, 4) and torch.isfinite(imgs).all()


@pytest.mark.parametrize("W,precision", [(64, None), (128, None)])
def test_fallback(fx, W, precision):
    """Networks the walk kernels do not serve - a default-precision model (`auto` resolves to int8 digits on init-law weights) and a width without a fused
    kernel: the C entry point answers SNERF_E_INVALID, the Python functions give the results of the loop over component_render_by_dir +
    get_imgs_from_Img_Dict_t_step."""
    sn, g = fx[0], fx[1]
    from season_nerf_amd import render as R_
    net = make_net(W, 4, 7, precision)
    L = sn._lib.lib()
    if W == 64:
        assert net.resolved_precision == "i8x3"
        z = torch.zeros(8, 3, device=DEV)
        tv = torch.zeros(4, device=DEV)
        fo = sn._lib.FieldOut()
        rc = L.snerf_field_sun_walk_rays(net.device_model(), 8, 4, z.data_ptr(), z.data_ptr(), tv.data_ptr(), 2, z.data_ptr(), None, C.byref(fo), None)
        assert rc == -1 and b"BF16X3" in L.snerf_last_error()
    else:
        assert not net.fused
        assert not L.snerf_model_create(W, 4)                     # no model exists at this width ...
        assert L.snerf_field_sun_walk_rays(None, 8, 4, None, None, None, 2, None, None, None, None) == -1      # ... and none is accepted
    assert not R_._walks(net)
    size, view, suns, times = (5, 6, 33), (70, 20), [(30, 90), (60, 200), (45, 300)], [0.1, 0.6]
    walk = sn.component_render_sun_walk(net, view, suns, times[0], size, g["WC"], g["H"], DEV)
    imgs, mask = sn.render_sun_season_walk(net, view, suns, times, size, g["WC"], g["H"], DEV)
    tim = torch.tensor(np.stack([sn.encode_time(t) for t in times]), dtype=torch.float32, device=DEV)
    cv = net.get_class_only(tim).cpu().numpy().astype(np.float64)
    for j, s in enumerate(suns):
        d = _single(sn, net, view, s, times[0], size, g)
        for k in ["World_Points", "Deltas", "Rho", "Base_Col", "Adjust_col", "Est_Solar_Vis", "Sky_Col", "Output_class"]:
            close(f"{k}[{j}]", walk[j][k], d[k], rtol=1e-4, atol=3e-5)
        close(f"imgs[{j}]", imgs[j].cpu().numpy(), sn.get_imgs_from_Img_Dict_t_step(d, size, cv), rtol=1e-4, atol=3e-5)
        close(f"mask[{j}]", mask[j].cpu().numpy(), sn.get_imgs_from_Img_Dict(d, size, False)["Shadow_Mask"], rtol=1e-4, atol=3e-5)


def test_opcheck_and_validation(fx):
    """torch.library.opcheck on the two ops at (4, 4, 24), M = 2, T = 2, and their argument checks."""
    sn, g, net = fx[0], fx[1], fx[2]
    from season_nerf_amd import render as R_
    ops = sn.ops.load()
    R, S, M, T = 16, 24, 2, 2
    walk = sn.component_render_sun_walk(net, (70, 20), [(30, 90), (60, 200)], 0.3, (4, 4, S), g["WC"], g["H"], DEV)
    d = walk.dev
    suns = torch.tensor(np.stack([sn.world_angle_2_local_vec(30, 90, g["WC"], g["H"]), sn.world_angle_2_local_vec(60, 200, g["WC"], g["H"])]),
                        dtype=torch.float32, device=DEV)
    h = net.device_model()
    args = (h, d["top"], d["bot"], d["tv"], suns, d["Class"])
    r = ops.sun_walk_fwd(*args)
    assert [tuple(t.shape) for t in r] == [(R, S, 1), (M, R, S, 1), (R, S, 3), (R, S, 4, 3), (R, S, 3)]
    assert torch.equal(r[1], d["Solar_Vis_All"]) and torch.equal(r[0], d["Rho"]) and torch.equal(r[3], d["Adjust_col"])
    torch.library.opcheck(torch.ops.season_nerf.sun_walk_fwd.default, args, test_utils=("test_schema", "test_faketensor"))
    cv = torch.rand(T, 4, device=DEV)
    cargs = (d["top"], d["bot"], d["tv"], d["Rho"], d["Base_Col"], d["Adjust_col"], d["Solar_Vis_All"], d["Sky_All"], cv, 2)
    o = ops.composite_sun_walk(*cargs)
    assert [tuple(t.shape) for t in o] == [(M, T, R, 3), (T, R, 3), (R, 3), (M, R), (M, R, 3)]
    assert torch.equal(o[0], R_._composite_sun_walk(d, cv)["shaded"])
    torch.library.opcheck(torch.ops.season_nerf.composite_sun_walk.default, cargs, test_utils=("test_schema", "test_faketensor"))
    torch.library.opcheck(torch.ops.season_nerf.composite_sun_walk.default, cargs + (d["Deltas"],), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError, match="suns"):
        ops.sun_walk_fwd(h, d["top"], d["bot"], d["tv"], suns[:, :2].contiguous(), None)
    with pytest.raises(RuntimeError, match="1 to 32"):
        ops.sun_walk_fwd(h, d["top"], d["bot"], d["tv"], suns[:1].expand(33, 3).contiguous(), None)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sun_walk_fwd(h, d["top"].cpu(), d["bot"], d["tv"], suns, None)
    with pytest.raises(RuntimeError, match="NULL"):
        ops.sun_walk_fwd(0, d["top"], d["bot"], d["tv"], suns, None)
    with pytest.raises(RuntimeError, match="R\\*S"):
        ops.composite_sun_walk(*cargs[:6], d["Solar_Vis_All"][:1].contiguous(), *cargs[7:])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.composite_sun_walk(*cargs[:7], d["Sky_All"].cpu(), *cargs[8:])
    with pytest.raises(RuntimeError, match="bot"):
        ops.composite_sun_walk(d["top"], d["bot"][:3].contiguous(), *cargs[2:])
