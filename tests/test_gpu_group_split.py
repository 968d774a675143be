"""GPU: the split per-ray kernel (csrc/kernels_group.hip: one 32-ray tile per workgroup, every layer's output blocks divided over the four waves) against
the one-wave kernel of the same arithmetic (mlp_kernel<PROG_GROUP>, csrc/kernels.hip), bit for bit.

An output block is computed by one wave, over the whole K, in the k-step order, product order and with the epilogue of the one-wave kernel; only WHICH wave
computes it, and that activations cross the waves through LDS, differs.  So all three outputs of snerf_group_forward (class weights, raw sky, sky) must be
`np.array_equal` between the two kernels (snerf_set_group_kernel: 0 = split, 1 = one wave):
  * at 1, 31, 32, 33 rays (partial tiles), 127, 128, 129 (the one-wave kernel's 128-ray tile edge) and 8192 + 33 (more 32-ray tiles than a 256-CU part has
    workgroups: some run a second tile, and the last tile is partial), at W = 256 and W = 64 (where two of the four waves own no block and only take the barriers);
  * with fewer classes than kMaxClasses (the softmax and the class store are masked by the class count);
  * with d_sky_raw or d_classes null (the optional outputs of the C ABI);
and two launches of the split kernel on the same inputs must be equal (a missing barrier around the activation buffers shows as run-to-run differences).
Every output buffer starts as NaN: an element that a kernel does not write fails the comparison with itself."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 127, 128, 129, 8192 + 33)
SPLIT, ONE_WAVE = 0, 1


def _inputs(n, seed):
    """Times and sun vectors as bench.py's synth draws them."""
    rng = np.random.Generator(np.random.PCG64(seed))
    sun = rng.uniform(0, 1, (n, 3))
    sun /= np.linalg.norm(sun, axis=1, keepdims=True)
    tau, d = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    tim = np.stack([np.cos(2 * np.pi * tau), np.sin(2 * np.pi * tau), np.cos(2 * np.pi * d), np.sin(2 * np.pi * d)], 1)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device="cuda")
    return t(tim), t(sun)


@pytest.fixture(scope="module")
def nets(golden_dir):
    """{name: (module, device model handle)}: the golden weights at both widths and a synthetic three-class network."""
    import season_nerf_amd as sn
    out = {}
    for key, name in (("W256", "net_W256_s1.npz"), ("W64", "net_W64_s0.npz")):
        g = np.load(os.path.join(golden_dir, name), allow_pickle=False)
        net = sn.T_NeRF(int(g["W"]), int(g["C"]))
        net.load_state_dict(orc.init_weights(int(g["W"]), int(g["C"]), int(g["seed"])))
        out[key] = net.to("cuda").eval()
    net = sn.T_NeRF(256, 3)
    net.load_state_dict(sn.synthetic_state_dict(net, 11))
    out["W256_C3"] = net.to("cuda").eval()
    yield {k: (n, n.device_model()) for k, n in out.items()}
    sn._lib.check(sn._lib.lib().snerf_set_group_kernel(SPLIT), "restore the default group kernel")


def _classes(L, model):
    return int(L.snerf_model_classes(model))


def group_forward(model, mode, tim, sun, want=("classes", "sky_raw", "sky")):
    """One snerf_group_forward with kernel `mode`; outputs not in `want` are passed as null.  Returns {name: numpy array}."""
    import season_nerf_amd as sn
    L = sn._lib.lib()
    n, c = tim.shape[0], _classes(L, model)
    sn._lib.check(L.snerf_set_group_kernel(mode), "snerf_set_group_kernel")
    bufs = {"classes": torch.full((n, c), float("nan"), device="cuda"), "sky_raw": torch.full((n, 3), float("nan"), device="cuda"),
            "sky": torch.full((n, 3), float("nan"), device="cuda")}
    ptr = lambda k: bufs[k].data_ptr() if k in want else None
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sn._lib.check(L.snerf_group_forward(model, n, tim.data_ptr(), sun.data_ptr(), ptr("classes"), ptr("sky_raw"), ptr("sky"), st), "group")
    torch.cuda.synchronize()
    return {k: bufs[k].cpu().numpy() for k in want}


def _compare(model, n, seed, want=("classes", "sky_raw", "sky")):
    tim, sun = _inputs(n, seed)
    ref = group_forward(model, ONE_WAVE, tim, sun, want)
    got = group_forward(model, SPLIT, tim, sun, want)
    again = group_forward(model, SPLIT, tim, sun, want)
    bad = []
    for k in want:
        assert not np.isnan(ref[k]).any(), (k, "the one-wave kernel left elements unwritten")
        d_ref, d_run = int((got[k] != ref[k]).sum()), int((got[k] != again[k]).sum())        # (NaN != NaN: an unwritten element counts)
        print(f"  n={n} {k:8s} split vs one wave: {d_ref} of {got[k].size} differ; split, two launches: {d_run} differ")
        if not np.array_equal(got[k], ref[k]):
            bad.append((k, "split != one wave", d_ref))
        if not np.array_equal(got[k], again[k]):
            bad.append((k, "two launches of the split kernel differ", d_run))
    assert not bad, bad


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key", ["W256", "W64"])
def test_split_kernel_equals_one_wave_kernel_bit_for_bit(nets, key, n):
    _compare(nets[key][1], n, 1000 + n)


def test_fewer_classes_than_the_maximum(nets):
    import season_nerf_amd as sn
    model = nets["W256_C3"][1]
    assert _classes(sn._lib.lib(), model) == 3
    _compare(model, 8192 + 33, 7)


@pytest.mark.parametrize("want", [("classes", "sky"), ("sky_raw", "sky")], ids=["sky_raw_null", "classes_null"])
@pytest.mark.parametrize("key", ["W256", "W64"])
def test_optional_output_pointers(nets, key, want):
    _compare(nets[key][1], 129, 5, want)


def test_mode_is_validated():
    import season_nerf_amd as sn
    L = sn._lib.lib()
    assert L.snerf_set_group_kernel(2) == -1 and b"snerf_set_group_kernel" in L.snerf_last_error()
    assert L.snerf_set_group_kernel(SPLIT) == 0
