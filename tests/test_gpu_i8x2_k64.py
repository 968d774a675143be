"""GPU: the two-wave int8 field kernel on v_mfma_i32_16x16x64_i8 (csrc/kernels_i8x2.hip run_layer16, W = 256) against the one-wave kernel
(csrc/kernels_i8.hip, v_mfma_i32_32x32x32_i8, its own weight stream), bit for bit.

The digits, scales and biases are the same integers and floats in both streams, integer accumulation is exact in any order, and the per-element
epilogue is the same sequence of operations, so every output must be `torch.equal`: variants 0, 1, 2 through snerf_field_forward_rays, variant 3 through
snerf_field_ray_visibility, one case through snerf_field_forward_points (points given, not generated from rays).  Shapes: 37 rays x 45 samples (1665
points: a ragged last tile, a ragged visibility group and pass), 3 x 96 (288 points: two tiles, the second with one wave's worth of points), 700 x 96
(263 tiles: just over one per CU, so the ring wraps across tiles on a few workgroups only).  Every launch is made twice and the two must be equal.
SNERF_I8_ONE_WAVE=1 selects the one-wave kernel and is read once per process, so the reference is a child process that saves its outputs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = 256
SIZES = ((37, 45), (3, 96), (700, 96))
POINTS = 1000                  # snerf_field_forward_points: 1000 points in groups of 7 (a ragged tile, groups that straddle waves)
CLASSES = 4
FIELD_OUTPUTS = {0: ("rho", "solar_vis", "col_raw", "adjust", "col", "adjust_col", "points"), 1: ("rho", "solar_vis", "points"), 2: ("rho", "points")}
FLOATS_PER_POINT = {"rho": 1, "solar_vis": 1, "col_raw": 3, "adjust": 3 * CLASSES, "col": 3, "adjust_col": 3, "points": 3}


def _model():
    import season_nerf_amd as sn
    net = sn.T_NeRF(W, CLASSES)
    net.load_state_dict(orc.init_weights(W, CLASSES, 21))
    net.precision = "i8x3"
    net = net.to("cuda").eval()
    return net, net.device_model()


def _inputs(R, S):
    import season_nerf_amd as sn
    rng = np.random.Generator(np.random.PCG64(1000 * R + S))
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32).cuda()
    top = t(np.concatenate([rng.uniform(-1, 1, (R, 2)), np.ones((R, 1))], 1))
    bot = t(np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1))
    sun = rng.uniform(0, 1, (R, 3))
    sun = t(sun / np.linalg.norm(sun, axis=1, keepdims=True))
    e = np.exp(rng.normal(size=(R, CLASSES)))
    cls = t(e / e.sum(1, keepdims=True))
    tv = sn.sample_parameters(S, eval_mode=True).cuda()
    return top, bot, sun, cls, tv


def _twice(names, n_points, launch):
    """two launches into NaN-filled buffers: all written, both equal; returns the first as cpu tensors"""
    runs = []
    for _ in range(2):
        bufs = {n: torch.full((n_points * FLOATS_PER_POINT[n],), float("nan"), device="cuda") for n in names}
        launch(bufs)
        torch.cuda.synchronize()
        runs.append(bufs)
    for n in names:
        assert not torch.isnan(runs[0][n]).any(), (n, "not written")
        assert torch.equal(runs[0][n], runs[1][n]), (n, "differs between two launches")
    return {n: runs[0][n].cpu() for n in names}


def ray_outputs(net_model, R, S):
    import season_nerf_amd as sn
    L = sn._lib.lib()
    _, model = net_model
    top, bot, sun, cls, tv = _inputs(R, S)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for variant, names in FIELD_OUTPUTS.items():
        def launch(bufs):
            fo = sn._lib.FieldOut(**{"d_" + n: b.data_ptr() for n, b in bufs.items()})
            sn._lib.check(L.snerf_field_forward_rays(model, variant, R, S, top.data_ptr(), bot.data_ptr(), tv.data_ptr(), 1, sun.data_ptr(), cls.data_ptr(),
                                                     C.byref(fo), st), "field")
        for n, v in _twice(names, R * S, launch).items():
            res[f"v{variant}_{n}"] = v
    for flags in (0, 2):
        runs = []
        for _ in range(2):
            vis = torch.full((R,), float("nan"), device="cuda")
            sn._lib.check(L.snerf_field_ray_visibility(model, R, S, top.data_ptr(), bot.data_ptr(), tv.data_ptr(), flags, vis.data_ptr(), st), "ray visibility")
            torch.cuda.synchronize()
            runs.append(vis)
        assert not torch.isnan(runs[0]).any(), ("vis", flags, "not written")
        assert torch.equal(runs[0], runs[1]), (R, S, "vis", flags, "differs between two launches")
        res[f"v3_vis_flags{flags}"] = runs[0].cpu()
    return res


def point_outputs(net_model):
    """variant 0 through snerf_field_forward_points: points beyond the cube, one sun / class row per group of 7 points"""
    import season_nerf_amd as sn
    L = sn._lib.lib()
    _, model = net_model
    rng = np.random.Generator(np.random.PCG64(77))
    G = -(-POINTS // 7)
    pts = torch.tensor(rng.uniform(-1.3, 1.3, (POINTS, 3)), dtype=torch.float32).cuda()
    sun = rng.uniform(0, 1, (G, 3))
    sun = torch.tensor(sun / np.linalg.norm(sun, axis=1, keepdims=True), dtype=torch.float32).cuda()
    e = np.exp(rng.normal(size=(G, CLASSES)))
    cls = torch.tensor(e / e.sum(1, keepdims=True), dtype=torch.float32).cuda()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def launch(bufs):
        fo = sn._lib.FieldOut(**{"d_" + n: b.data_ptr() for n, b in bufs.items()})
        sn._lib.check(L.snerf_field_forward_points(model, 0, POINTS, pts.data_ptr(), 7, sun.data_ptr(), cls.data_ptr(), C.byref(fo), st), "field points")
    return {f"points_v0_{n}": v for n, v in _twice(FIELD_OUTPUTS[0], POINTS, launch).items()}


def dump_all(path):
    """The child process's job: all cases with the kernel the environment selects."""
    nm = _model()
    out = {(R, S): ray_outputs(nm, R, S) for R, S in SIZES}
    out["points"] = point_outputs(nm)
    torch.save(out, path)


@pytest.fixture(scope="module")
def one_wave(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("one_wave_k64") / "outputs.pt")
    code = ("import os, sys; sys.path.insert(0, os.getcwd()); import tests.test_gpu_i8x2_k64 as t; "
            f"t.dump_all({path!r}); print('ONE_WAVE_DONE')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SNERF_I8_ONE_WAVE="1"), capture_output=True, text=True, timeout=600)
    print(r.stdout[-600:], r.stderr[-2000:])
    assert r.returncode == 0 and "ONE_WAVE_DONE" in r.stdout
    return torch.load(path)


@pytest.fixture(scope="module")
def net_model():
    assert os.environ.get("SNERF_I8_ONE_WAVE") is None and os.environ.get("SNERF_I8X2_MFMA32") is None, "this process must run the 16x16x64 two-wave kernel"
    return _model()


def _compare(got, ref, what):
    assert sorted(got) == sorted(ref)
    bad = []
    for k in sorted(got):
        same = torch.equal(got[k], ref[k])
        n_diff = 0 if same else int((got[k] != ref[k]).sum())
        print(f"  {what} {k:20s} {'equal' if same else f'{n_diff} of {got[k].numel()} elements differ'}")
        if not same:
            bad.append((k, n_diff))
    assert not bad, bad


@pytest.mark.parametrize("R,S", SIZES)
def test_k64_kernel_equals_one_wave_kernel_bit_for_bit(one_wave, net_model, R, S):
    got = ray_outputs(net_model, R, S)
    assert len(got) == 7 + 3 + 2 + 2
    _compare(got, one_wave[(R, S)], f"{R}x{S}")


def test_k64_kernel_equals_one_wave_kernel_on_given_points(one_wave, net_model):
    got = point_outputs(net_model)
    assert len(got) == 7
    _compare(got, one_wave["points"], "points")
