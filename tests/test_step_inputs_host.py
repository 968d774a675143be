"""step_inputs.DeviceStepInputs on the host (no GPU): the mirror of the device draw against the reference-pinned arithmetic, the law of the sun rays and
the jitter on N = 100003 rays, the separation of the stream from the loader's and across draws and ranks, the schedule table against real Net_tool
optimisers and schedulers, and the argument errors of the C ABI (raised before anything touches a GPU).

The statistical bounds are conditions set in advance: a 16-bin histogram count of N uniform draws has standard deviation sqrt(N * 15 / 256) (5 sigma: 8 * 16
bins at 5.7e-7 each), the sample correlation of two independent streams 1 / sqrt(N) (28 pairs at 5 sigma) - together about 1e-4 for a correct generator.  A
failure is a finding about the word assignment, not a reason to change the seed."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

N = 100003
SEED = 20240917
WC = np.array([41.29, -95.9, 300.0])
H_LOADER = np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])      # the loader tests' matrix
# geodetic scale: ~333 and ~250 cube units per degree about the centre, 1 / 150 per metre
H_GEO = np.array([[333.0, 0.0, 0.0, -333.0 * 41.29], [0.0, 250.0, 0.0, 250.0 * 95.9], [0.0, 0.0, 1.0 / 150.0, -2.0], [0, 0, 0, 1.0]])
MATRICES = {"loader": H_LOADER, "geodetic": H_GEO}


@pytest.fixture(scope="module")
def SI():
    from season_nerf_amd import step_inputs
    return step_inputs


@pytest.fixture(scope="module")
def big(SI):
    """Draw 0 of N rays and N samples under the fixed seed, per matrix: the mirror's arrays and the eight uniform streams (read-only, shared)."""
    out = {}
    for name, H in MATRICES.items():
        di = SI.DeviceStepInputs({"W2L_H": H, "WC": WC}, N, N, SEED)
        m = di.host_mirror(0)
        for v in m.values():
            v.setflags(write=False)
        out[name] = (di, m)
    out["uniforms"] = SI.host_uniforms(SEED, 0, 0, N, N)
    return out


@pytest.mark.parametrize("name", list(MATRICES))
def test_mirror_vec_is_the_reference_pinned_arithmetic_bit_for_bit(big, name):
    from season_nerf_amd.training import _angles_to_local_vecs
    _, m = big[name]
    vec64 = _angles_to_local_vecs(m["az_el"][:, 1], m["az_el"][:, 0], WC, MATRICES[name])
    assert vec64.dtype == np.float64 and np.array_equal(vec64.astype(np.float32), m["vec"])
    ends = (m["starts"].astype(np.float64) - 2 * (vec64 / vec64[:, 2:])).astype(np.float32)
    assert ends.tobytes() == m["ends"].tobytes()


def test_world_angle_2_local_vec_recorded_value():
    """SURVEY's recorded value of the reference's world_angle_2_local_vec(60, 30, centre, identity)."""
    from season_nerf_amd.training import _angles_to_local_vecs
    v = _angles_to_local_vecs(np.array([60.0]), np.array([30.0]), WC, np.eye(4))[0]
    np.testing.assert_allclose(v, [0.0352731, -0.0819149, 0.99601494], atol=1e-7)


def test_host_generator_is_the_one_law_function_bitwise():
    """create_solor_rays_uniform draws what it always drew (numpy, torch, torch, torch in that order) and runs the shared law on them, fp32 cos included."""
    import season_nerf_amd as sn
    from season_nerf_amd.training import _angles_to_local_vecs
    n = 257
    np.random.seed(5); torch.manual_seed(5)
    st, en, ve, ti, ae = sn.create_solor_rays_uniform(H_LOADER, WC)(n, include_times=True)
    np.random.seed(5); torch.manual_seed(5)
    az_el = np.random.random(n * 2).reshape([n, 2]) * np.array([[360, 89]]) + np.array([[-180, 1]])
    vec = _angles_to_local_vecs(az_el[:, 1], az_el[:, 0], WC, H_LOADER)
    starts = np.ones([n, 3], dtype=np.float32)
    starts[:, 0] = np.float32(2.0) * torch.rand(n).numpy() + np.float32(-1.0)
    starts[:, 1] = np.float32(2.0) * torch.rand(n).numpy() + np.float32(-1.0)
    ends = (starts.astype(np.float64) - 2 * (vec / vec[:, 2::])).astype(np.float32)
    fr = torch.rand([n, 2]).numpy() * np.float32(2 * np.pi)
    times = np.stack([np.cos(fr[:, 0]), np.sin(fr[:, 0]), np.cos(fr[:, 1]), np.sin(fr[:, 1])], 1).astype(np.float32)
    assert fr.dtype == np.float32
    assert np.array_equal(ae, az_el) and st.numpy().tobytes() == starts.tobytes() and en.numpy().tobytes() == ends.tobytes()
    assert ve.numpy().tobytes() == vec.astype(np.float32).tobytes() and ti.numpy().tobytes() == times.tobytes()


@pytest.mark.parametrize("name", list(MATRICES))
def test_law_of_the_sun_rays(big, name):
    _, m = big[name]
    az, el = m["az_el"][:, 0], m["az_el"][:, 1]
    assert az.min() >= -180 and az.max() < 180 and el.min() >= 1 and el.max() < 90
    st, en, vec = m["starts"], m["ends"], m["vec"]
    assert st[:, :2].min() >= -1 and st[:, :2].max() < 1 and np.all(st[:, 2] == 1)
    assert np.all(en[:, 2] == -1)
    nrm = np.sqrt((vec.astype(np.float64) ** 2).sum(1))
    assert np.abs(nrm - 1).max() <= 2.0 ** -23 and vec[:, 2].min() > 0
    t = m["times"].astype(np.float64)
    assert np.abs(t[:, 0] ** 2 + t[:, 1] ** 2 - 1).max() < 1e-6 and np.abs(t[:, 2] ** 2 + t[:, 3] ** 2 - 1).max() < 1e-6


def test_histograms_and_correlations_of_the_eight_streams(big, SI):
    di, m = big["loader"]
    base, S = SI.jitter_base(N), N
    ang = lambda c, s: np.mod(np.arctan2(s.astype(np.float64), c.astype(np.float64)), 2 * np.pi) / (2 * np.pi)
    streams = {"az": (m["az_el"][:, 0] + 180) / 360, "el": (m["az_el"][:, 1] - 1) / 89, "x": (m["starts"][:, 0].astype(np.float64) + 1) / 2,
               "y": (m["starts"][:, 1].astype(np.float64) + 1) / 2, "t0": ang(m["times"][:, 0], m["times"][:, 1]), "t1": ang(m["times"][:, 2], m["times"][:, 3]),
               # (at S = N the sum base + u / S keeps ~7 bits of u: the jitter's histogram is taken on the uniforms, which the sums below are built from bit for bit)
               "jitter_image": big["uniforms"]["jitter_image"].astype(np.float64), "jitter_solar": big["uniforms"]["jitter_solar"].astype(np.float64)}
    sigma = np.sqrt(N * 15 / 256)
    for k, u in streams.items():
        assert u.min() >= 0 and u.max() < 1 + 1e-9, k
        h = np.bincount(np.clip((u * 16).astype(int), 0, 15), minlength=16)
        assert np.abs(h - N / 16).max() <= 5 * sigma, (k, h)
    U = big["uniforms"]
    names = list(U)
    assert len(names) == 8
    cc = np.corrcoef(np.stack([U[k].astype(np.float64) for k in names]))
    off = np.abs(cc - np.eye(8)).max()
    assert off < 5 / np.sqrt(N), (off, cc)
    # the mirror's outputs are those uniforms under the law
    assert np.array_equal(m["az_el"][:, 0], U["az"] * 360 + -180) and np.array_equal(m["az_el"][:, 1], U["el"] * 89 + 1) and m["starts"][:, 0].tobytes() == (np.float32(2.0) * U["x"] + np.float32(-1.0)).tobytes()
    assert m["tv_image"].tobytes() == (base + np.float32(1.0 / S) * U["jitter_image"]).tobytes()
    assert m["tv_solar"].tobytes() == (base + np.float32(1.0 / S) * U["jitter_solar"]).tobytes()
    assert m["tv_image"].min() >= 0 and m["tv_image"].max() <= 1 and np.all(np.diff(m["tv_image"].astype(np.float64)) > -1.0 / S)


def test_stream_separation(SI):
    from season_nerf_amd import loader
    rw, sw = SI.host_words(SEED, 0, 0, 1024, 64)
    top, bot = loader.host_sc_rays(SEED, 0, 0, 0, 1024)
    mine = np.float32(2.0) * SI._u24(rw[:, :4]) + np.float32(-1.0)                    # the loader's law on this stream's first 4096 words
    theirs = np.concatenate([top[:, :2], bot[:, :2]], 1)
    assert (mine == theirs).sum() <= 1                                               # (24-bit values: one chance agreement in 4096 has probability 2.4e-4)
    rw1, sw1 = SI.host_words(SEED, 1, 0, 1024, 64)
    rwr, swr = SI.host_words(SEED, 0, 1, 1024, 64)
    rws, _ = SI.host_words(SEED + 1, 0, 0, 1024, 64)
    for a, b in ((rw, rw1), (rw, rwr), (rw, rws), (sw, sw1), (sw, swr), (rw[:, :4], rw[:, 4:]), (rw[:64, :4], sw), (rw[:64, 4:], sw)):
        assert (a == b).sum() == 0
    again = SI.host_words(SEED, 0, 0, 1024, 64)
    assert np.array_equal(rw, again[0]) and np.array_equal(sw, again[1])
    # the generator under the documented key and counters
    k = _splitmix64(SEED ^ 0x73746570696e7031)
    for blk, idx, want in ((0, 5, rw[5, :4]), (1, 1023, rw[1023, 4:]), (2, 63, sw[63])):
        got = loader.philox4x32_10([idx, 0, 0, 0 + (blk << 24)], [k & 0xffffffff, k >> 32])
        assert np.array_equal(got, want), (blk, idx)
    got = loader.philox4x32_10([7, 3, 1, 9 + (2 << 24)], [k & 0xffffffff, k >> 32])
    assert np.array_equal(got, SI.host_words(SEED, 3 + (1 << 32), 9, 1, 8)[1][7])


def _splitmix64(z):
    M = (1 << 64) - 1
    z = (z + 0x9e3779b97f4a7c15) & M
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M
    return z ^ (z >> 31)


def _tool(use_mse, use_prior, n_phase_steps, total, lr, scale):
    """A real Net_tool on the CPU (its optimisers and schedulers are host objects); the adaptive-loss objects are stand-ins with parameters."""
    import season_nerf_amd as sn
    args = SimpleNamespace(n_samples=8, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=use_mse, Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=4)
    ada = None if use_mse else ([torch.nn.Linear(1, 1), torch.nn.Linear(1, 1)] if use_prior else torch.nn.Linear(1, 1))
    ev = sn.All_in_One_Eval(args, torch.device("cpu"), n_phase_steps, use_prior, ada, H_LOADER, WC)
    net = sn.T_NeRF(64, 4)
    tool = sn.Net_tool(net, ev, lr, total_steps=total, lr_alpha_scale=scale, writer=None)
    net._param_store = SimpleNamespace(adam_steps=0)           # what FusedAdam.next_hyper counts its steps in (no engine on the CPU)
    return tool


@pytest.mark.parametrize("use_mse,use_prior,first", [(True, False, 0), (False, True, 37)])
def test_schedule_table_equals_what_a_net_tool_produces(SI, use_mse, use_prior, first):
    total, n_phase = 240, 400
    tool = _tool(use_mse, use_prior, n_phase, total, 10 ** -4.86 * 3, 1000.0)
    assert (tool.optim2 is None) == use_mse
    di = SI.DeviceStepInputs(tool, 16, 8, seed=1, first_step=first)
    tab = di.table_host
    assert tab.shape == (total, 8) and tab.dtype == np.float32
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in range(total):
            hyper = torch.tensor(tool.optim.next_hyper(), dtype=torch.float32).numpy()                  # as GraphedTrainStep._load / set_hyper upload it
            trust = torch.tensor([(first + k) / tool.eval_tool.n_steps], dtype=torch.float32).numpy()      # Eval_Tools_2.py:243 through _load
            assert tab[k, :6].tobytes() == hyper.tobytes() and tab[k, 6:7].tobytes() == trust.tobytes(), k
            if tool.optim2 is not None:
                lr2 = torch.full((), float(tool.optim2.param_groups[0]["lr"]), dtype=torch.float32).numpy()
                assert tab[k, 7].tobytes() == lr2.tobytes(), k
            if k + 1 < total:
                tool.sched.step()
                if tool.sched2 is not None:
                    tool.sched2.step()
    assert len(set(tab[:, 0])) > total // 2 and tab[0, 4] == np.float32(1.0 - 0.9)
    m = di.host_mirror(3, step=10 ** 9)                        # past the last row: the last row
    assert m["hyper"].tobytes() == tab[-1, :6].tobytes() and m["lr2"][0] == tab[-1, 7]


def test_c_abi_refuses_bad_arguments_without_a_gpu():
    import season_nerf_amd as sn
    lib = sn._lib.lib()
    INVALID = -1
    H, wc = np.ascontiguousarray(H_LOADER), np.ascontiguousarray(WC)
    tab = np.zeros((4, 8), dtype=np.float32)                  # an address that is never read: every call below is refused first or touches no device
    h = C.c_void_p()
    ok = dict(seed=1, n_rays=8, n_samples=4, rank=0, H=H.ctypes.data, wc=wc.ctypes.data, tab=tab.ctypes.data, rows=4, out=C.byref(h))
    call = lambda **kw: lib.snerf_step_inputs_create(*[dict(ok, **kw)[k] for k in ("seed", "n_rays", "n_samples", "rank", "H", "wc", "tab", "rows", "out")])
    bad_H, bad_wc = H.copy(), wc.copy()
    bad_H[1, 2], bad_wc[0] = np.inf, np.nan
    for kw in (dict(H=None), dict(wc=None), dict(tab=None), dict(out=None), dict(n_rays=0), dict(n_samples=0), dict(n_rays=-3), dict(rank=-1), dict(rank=1 << 24),
               dict(H=bad_H.ctypes.data), dict(wc=bad_wc.ctypes.data), dict(rows=0), dict(rows=-1)):
        assert call(**kw) == INVALID, kw
        assert not h.value and lib.snerf_last_error(), kw
    assert call(rank=(1 << 24) - 1) == 0 and h.value
    s, back = np.array([5, 3, 0, 0], dtype=np.int64), np.zeros(4, dtype=np.int64)
    try:
        assert lib.snerf_step_inputs_rays(h) == 8 and lib.snerf_step_inputs_samples(h) == 4 and lib.snerf_step_inputs_table_rows(h) == 4
        assert lib.snerf_step_inputs_get_state(h, back.ctypes.data, None) == 0 and not back.any()
        assert lib.snerf_step_inputs_set_state(h, s.ctypes.data, None) == 0                       # the shadow: no draw has allocated the device copy
        assert lib.snerf_step_inputs_get_state(h, back.ctypes.data, None) == 0 and np.array_equal(back, s)
        for bad in ([-1, 0, 0, 0], [0, -1, 0, 0]):
            b = np.array(bad, dtype=np.int64)
            assert lib.snerf_step_inputs_set_state(h, b.ctypes.data, None) == INVALID
        assert lib.snerf_step_inputs_get_state(h, back.ctypes.data, None) == 0 and np.array_equal(back, s)
        assert lib.snerf_step_inputs_draw(h, None, None) == INVALID and lib.snerf_step_inputs_draw(None, None, None) == INVALID
        assert lib.snerf_step_inputs_get_state(None, back.ctypes.data, None) == INVALID and lib.snerf_step_inputs_set_state(h, None, None) == INVALID
    finally:
        lib.snerf_step_inputs_destroy(h)
    w = np.zeros((2, 8), dtype=np.uint32)
    assert lib.snerf_step_inputs_words_host(1, -1, 0, 2, 0, w.ctypes.data, None) == INVALID
    assert lib.snerf_step_inputs_words_host(1, 0, 1 << 24, 2, 0, w.ctypes.data, None) == INVALID
    assert lib.snerf_step_inputs_words_host(1, 0, 0, 2, 0, None, None) == INVALID
    assert lib.snerf_step_inputs_words_host(1, 0, 0, 2, 0, w.ctypes.data, None) == 0 and w.any()


def test_python_object_state_round_trip_and_checks(SI):
    di = SI.DeviceStepInputs({"W2L_H": H_LOADER, "WC": WC}, 8, 4, seed=3, rank=2)
    assert di.get_state() == (0, 0)
    di.set_state(11, 4)
    sd = di.state_dict()
    assert sd == {"seed": 3, "rank": 2, "state": [11, 4, 0, 0]}
    other = SI.DeviceStepInputs({"W2L_H": H_LOADER, "WC": WC}, 8, 4, seed=3, rank=2)
    other.load_state_dict(sd)
    assert other.get_state() == (11, 4)
    with pytest.raises(ValueError, match="seed"):
        SI.DeviceStepInputs({"W2L_H": H_LOADER, "WC": WC}, 8, 4, seed=4, rank=2).load_state_dict(sd)
    with pytest.raises(RuntimeError, match="2\\^24"):
        SI.DeviceStepInputs({"W2L_H": H_LOADER, "WC": WC}, 8, 4, seed=3, rank=1 << 24)
    with pytest.raises(ValueError, match="step 7"):
        other.check_step(7)
    other.first_step = 3
    other.check_step(7)
    import season_nerf_amd as sn
    assert sn.DeviceStepInputs is SI.DeviceStepInputs and hasattr(sn.ops.load(), "step_inputs_draw")
