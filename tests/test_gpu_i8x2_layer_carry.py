"""GPU: the two-wave int8 field kernel (csrc/kernels_i8x2.hip) against the one-wave kernel of the same arithmetic (csrc/kernels_i8.hip), bit for bit.

The two-wave kernel finishes a layer's last block inside the next layer's first block (run_layer8x2: PEND / HANDOFF); only the place of that
epilogue in the instruction stream differs from the one-wave kernel, never a sum, an fma, a sine or a digit.  So every output of every variant must be
`torch.equal` between the two: variants 0, 1, 2 through snerf_field_forward_rays, variant 3 through snerf_field_ray_visibility, at W = 64 and 256, for
4096 x 96 points (six tiles per workgroup: the weight ring wraps around across tiles and layers) and for a ragged size (37 rays x 45 samples: 1665 points,
not a multiple of the 256-point tile; 37 rays, not a multiple of the eight rays of a visibility group; a ragged second pass).  Each launch is made twice and
the two launches are equal too.  SNERF_I8_ONE_WAVE=1 selects the one-wave kernel and is read once per process, so the reference is a child process that
saves its outputs."""
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
WIDTHS = (64, 256)
SIZES = ((4096, 96), (37, 45))
CLASSES = 4
FIELD_OUTPUTS = {0: ("rho", "solar_vis", "col_raw", "adjust", "col", "adjust_col", "points"), 1: ("rho", "solar_vis", "points"), 2: ("rho", "points")}
FLOATS_PER_POINT = {"rho": 1, "solar_vis": 1, "col_raw": 3, "adjust": 3 * CLASSES, "col": 3, "adjust_col": 3, "points": 3}


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


def field_outputs(W, R, S):
    """Every output of variants 0-3 of the i8x3 field kernel this process selects, as {name: cpu tensor}; each launch made twice and compared."""
    import season_nerf_amd as sn
    L = sn._lib.lib()
    net = sn.T_NeRF(W, CLASSES)
    net.load_state_dict(orc.init_weights(W, CLASSES, 21))
    net.precision = "i8x3"
    net = net.to("cuda").eval()
    model = net.device_model()
    top, bot, sun, cls, tv = _inputs(R, S)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    res = {}
    for variant, names in FIELD_OUTPUTS.items():
        runs = []
        for _ in range(2):
            bufs = {n: torch.full((R * S * FLOATS_PER_POINT[n],), float("nan"), device="cuda") for n in names}
            fo = sn._lib.FieldOut(**{"d_" + n: b.data_ptr() for n, b in bufs.items()})
            sn._lib.check(L.snerf_field_forward_rays(model, variant, R, S, top.data_ptr(), bot.data_ptr(), tv.data_ptr(), 1, sun.data_ptr(), cls.data_ptr(),
                                                     C.byref(fo), st), "field")
            torch.cuda.synchronize()
            runs.append(bufs)
        for n in names:
            assert not torch.isnan(runs[0][n]).any(), (variant, n, "not written")
            assert torch.equal(runs[0][n], runs[1][n]), (W, R, S, variant, n, "differs between two launches")
            res[f"v{variant}_{n}"] = runs[0][n].cpu()
    for flags in (0, 2):
        runs = []
        for _ in range(2):
            vis = torch.full((R,), float("nan"), device="cuda")
            sn._lib.check(L.snerf_field_ray_visibility(model, R, S, top.data_ptr(), bot.data_ptr(), tv.data_ptr(), flags, vis.data_ptr(), st), "ray visibility")
            torch.cuda.synchronize()
            runs.append(vis)
        assert not torch.isnan(runs[0]).any(), ("vis", flags, "not written")
        assert torch.equal(runs[0], runs[1]), (W, R, S, "vis", flags, "differs between two launches")
        res[f"v3_vis_flags{flags}"] = runs[0].cpu()
    return res


def dump_all(path):
    """The child process's job: all cases with the kernel the environment selects."""
    torch.save({(W, R, S): field_outputs(W, R, S) for W in WIDTHS for R, S in SIZES}, path)


@pytest.fixture(scope="module")
def one_wave(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("one_wave") / "outputs.pt")
    code = ("import os, sys; sys.path.insert(0, os.getcwd()); import tests.test_gpu_i8x2_layer_carry as t; "
            f"t.dump_all({path!r}); print('ONE_WAVE_DONE')")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, SNERF_I8_ONE_WAVE="1"), capture_output=True, text=True, timeout=900)
    print(r.stdout[-600:], r.stderr[-2000:])
    assert r.returncode == 0 and "ONE_WAVE_DONE" in r.stdout
    return torch.load(path)


@pytest.mark.parametrize("R,S", SIZES)
@pytest.mark.parametrize("W", WIDTHS)
def test_two_wave_kernel_equals_one_wave_kernel_bit_for_bit(one_wave, W, R, S):
    assert os.environ.get("SNERF_I8_ONE_WAVE") is None, "this process must run the two-wave kernel"
    ref = one_wave[(W, R, S)]
    got = field_outputs(W, R, S)
    assert sorted(got) == sorted(ref) and len(got) == 7 + 3 + 2 + 2
    bad = []
    for k in sorted(got):
        same = torch.equal(got[k], ref[k])
        n_diff = 0 if same else int((got[k] != ref[k]).sum())
        print(f"  W={W} {R}x{S} {k:16s} {'equal' if same else f'{n_diff} of {got[k].numel()} elements differ'}")
        if not same:
            bad.append((k, n_diff))
    assert not bad, bad
