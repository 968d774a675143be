"""GPU tests of the film-frame feature: `season_nerf::frame_walk` (csrc/mlp_device.h RayFrame; frame_walk_kernel<64|256>, frame_walk_ks_kernel<512>)
against the per-sample path (`forward_seperate` on the same float32 points, float64 sums), its early-out, one launch of T seasons against T launches of
one, the reference's recorded frames (tests/golden/movie_frames.npz), `get_Img`, the fallback, and the op's schema, fake kernel and argument checks.

Tolerance of the kernel tests: the measured rule of test_gpu_compositing.py (`_check`): each output within 4 * (E_ref + 2^-24 * scale), E_ref = the
deviation of the same formulas in CPU fp32 from float64; scale = 1 for the colours, sum PS and sum PS vis, S - 1 for sum PS s (the rule on the sum divided
by S - 1, at unit scale), the ray's optical depth for the depth walked.

Against the reference: E_FRAME of tests/test_frame_host.py, measured by `test_per_sample_deviation` below; the walk within 2 E_FRAME + 4 * 2^-24 * scale."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc
from test_frame_host import E_FRAME, EPS, MAX_T, direct_composite, fixture, frame_params, oracle_per_sample
from test_gpu_compositing import SENT, _check, _report
from test_gpu_surface import net_of, rays
from test_surface_host import TAGS, lattice, oracle_density, weights

pytestmark = pytest.mark.gpu
DEV = "cuda"
SUN = (0.3, -0.2, 0.93)
TIMES = (0.1, 0.45, 0.8, 0.62, 0.27, 0.93, 0.01)


def frame_rays(R, seed):
    """R parallel-slab style rays of one length (a frame has one delta): the even ones stand upright inside the cube, the odd ones are tilted and start
    near a face, so that they leave the cube: about half of the rays."""
    rng = np.random.Generator(np.random.PCG64(seed))
    L = 0.95
    odd = (np.arange(R) % 2 == 1)[:, None]
    c = np.where(odd, np.concatenate([rng.uniform(0.7, 0.95, (R, 1)), rng.uniform(-0.9, 0.9, (R, 1))], 1), rng.uniform(-0.9, 0.9, (R, 2)))
    c = np.concatenate([c, rng.uniform(-0.04, 0.04, (R, 1))], 1)
    v = np.where(odd, np.array([[0.5, -0.3, np.sqrt(1 - 0.34)]]), np.array([[0.0, 0.0, 1.0]]))
    f = lambda a: torch.tensor(a, dtype=torch.float32, device=DEV).contiguous()
    return f(c + L * v), f(c - L * v)


def group_inputs(net, times):
    """Sun direction, its sky colour and the class vectors of `times` from the network's own group network."""
    import season_nerf_amd as sn
    sun = torch.tensor(np.asarray(SUN) / np.sqrt(np.sum(np.asarray(SUN) ** 2)), dtype=torch.float32, device=DEV)
    tim = torch.tensor(np.stack([sn.encode_time(t) for t in times]), dtype=torch.float32, device=DEV)
    with torch.no_grad():
        cls, _, sky = net._groups(tim, sun.reshape(1, 3).expand(len(times), 3).contiguous())
    return sun, sky[0].contiguous(), cls.contiguous()


def per_sample(net, top, bot, tv, sun):
    """The per-sample path: `forward_seperate` on the points top (1 - t) + bot t -> rho [R,S], col_raw [R,S,3], vis [R,S], adj [R,S,C,3] (fp32, CPU) and
    the samples outside the cube [R,S]."""
    R, S = top.shape[0], tv.numel()
    t = tv.reshape(1, S, 1)
    pts = top.unsqueeze(1) * (1 - t) + bot.unsqueeze(1) * t
    with torch.no_grad():
        rho, col_raw, vis, _, _, adj = net.forward_seperate(pts.reshape(-1, 3), sun.reshape(1, 3).expand(R * S, 3), torch.zeros(R * S, 4, device=DEV))
    c = lambda a, *s: a.detach().reshape(R, S, *s).cpu()
    return c(rho), c(col_raw, 3), c(vis), c(adj, net.n_classes, 3), (pts.abs() > 1).any(2).cpu()


def statement(rho, col_raw, vis, adj, sky, cls, delta):
    """The sixteen sums in the dtype of the arguments (delta [R,S]: 0 where a sample does not count); PV as get_PV forms it."""
    y = rho * delta
    c = torch.cumsum(torch.cat([torch.zeros_like(y[:, :1]), y], 1), 1)
    ps = orc.get_PV(rho, delta) * (1 - torch.exp(-y))
    out = torch.zeros(rho.shape[0], 16, dtype=rho.dtype)
    shade = vis.unsqueeze(2) + (1 - vis.unsqueeze(2)) * sky.reshape(1, 1, 3)
    for k in range(cls.shape[0]):
        col = torch.sigmoid(col_raw + (adj * cls[k].reshape(1, 1, -1, 1)).sum(2))
        out[:, 3 * k:3 * k + 3] = (ps.unsqueeze(2) * shade * col).sum(1)
    out[:, 12], out[:, 13], out[:, 14], out[:, 15] = ps.sum(1), (ps * torch.arange(rho.shape[1], dtype=rho.dtype)).sum(1), c[:, -1], (ps * vis).sum(1)
    return out


def check_sixteen(kernel, family, got, ps_out, sky, cls, delta):
    """got [R,16] (fp32) against the float64 statement on the per-sample path's outputs, by the rule in the module docstring."""
    rho, col_raw, vis, adj = ps_out
    S, T = rho.shape[1], cls.shape[0]
    got = got.detach().cpu()
    d = lambda a: a.double()
    ref64 = statement(d(rho), d(col_raw), d(vis), d(adj), d(sky.cpu()), d(cls.cpu()), d(delta))
    ref32 = statement(rho, col_raw, vis, adj, sky.cpu(), cls.cpu(), delta)
    assert bool((got[:, 3 * T:12] == 0).all()), f"{kernel}/{family}: the slots of unused seasons are not 0"
    _check(kernel, family, "rgb", got[:, :3 * T], ref64[:, :3 * T], ref32[:, :3 * T], unit_scale=True)
    _check(kernel, family, "acc", got[:, 12], ref64[:, 12], ref32[:, 12], unit_scale=True)
    _check(kernel, family, "mi", got[:, 13] / (S - 1), ref64[:, 13] / (S - 1), ref32[:, 13] / (S - 1), unit_scale=True)
    _check(kernel, family, "carry", got[:, 14], ref64[:, 14], ref32[:, 14])
    _check(kernel, family, "psv", got[:, 15], ref64[:, 15], ref32[:, 15], unit_scale=True)


def launch(net, top, bot, tv, delta, sun, sky, cls, flags, pad=4):
    """snerf_field_frame_walk into a buffer with sentinel rows in front of and behind the output -> [R,16] (CPU)."""
    import season_nerf_amd as sn
    L = sn._lib.lib()
    n = top.shape[0]
    buf = torch.full(((n + 2 * pad) * 16,), SENT, device=DEV)
    assert buf.data_ptr() % 64 == 0
    rc = L.snerf_field_frame_walk(C.c_void_p(net.device_model()), n, tv.numel(), top.data_ptr(), bot.data_ptr(), tv.data_ptr(), C.c_float(delta), sun.data_ptr(),
                                  sky.data_ptr(), cls.shape[0], cls.data_ptr(), flags, buf.data_ptr() + pad * 64, C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.snerf_last_error()
    torch.cuda.synchronize()
    b = buf.cpu().reshape(n + 2 * pad, 16)
    assert bool((b[:pad] == SENT).all()) and bool((b[n + pad:] == SENT).all()), "a row outside the output was written"
    assert not bool((b[pad:n + pad] == SENT).any()), f"rows left unwritten: {torch.nonzero((b[pad:n + pad] == SENT).any(1)).reshape(-1).tolist()}"
    return b[pad:n + pad]


@pytest.mark.parametrize("S", [2, 31, 32, 33, 96])
@pytest.mark.parametrize("W", [64, 256, 512])
def test_kernel_vs_per_sample_path(golden_dir, W, S):
    """The kernel against the parent's per-sample path, early-out off; no reference involved.  R in {1, 5, 37}, T in {1, 3, MAX_T}, both settings of
    flags bit 1; unused season slots exactly 0, sentinels around the output untouched."""
    from season_nerf_amd.evaluator import sample_parameters_on
    net = net_of(golden_dir, f"sharp_W{W}")
    assert net.resolved_precision == "bf16x3"
    tv = sample_parameters_on(torch.device(DEV), S, eval_mode=True, include_end_pt=True)
    for R in (1, 5, 37):
        top, bot = frame_rays(R, 1000 * W + 10 * R + S)
        delta = float(torch.sqrt(((top[0] - bot[0]).double() ** 2).sum())) / (S - 1)
        rho, col_raw, vis, adj, oob = per_sample(net, top, bot, tv, group_inputs(net, TIMES[:1])[0])
        share = float(oob.any(1).float().mean())
        assert R < 5 or 0.3 <= share <= 0.7, share
        for T in (1, 3, MAX_T):
            sun, sky, cls = group_inputs(net, TIMES[:T])
            for zero_oob in (False, True):
                dl = torch.full((R, S), delta, dtype=torch.float32)
                if zero_oob:
                    dl = torch.where(oob, torch.zeros_like(dl), dl)
                got = launch(net, top, bot, tv, delta, sun, sky, cls, 4 | (2 if zero_oob else 0))
                assert bool(torch.isfinite(got).all())
                check_sixteen("frame_walk", f"W{W}", got, (rho, col_raw, vis, adj), sky, cls, dl)
    _report("frame_walk")


@pytest.mark.parametrize("W,rays_per_tile", [(64, 4), (512, 2)])
def test_persistent_loop_and_tile_tail(golden_dir, W, rays_per_tile):
    """More tiles than workgroups and a last tile with one ray: every row written, two launches bit for bit, the first rows as in a launch of those
    rays alone (early-out off: with it, which passes a ray skips depends on the rays it shares a workgroup with)."""
    from season_nerf_amd.evaluator import sample_parameters_on
    net = net_of(golden_dir, f"sharp_W{W}")
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    R, S = rays_per_tile * (n_cu + 3) + 1, 33
    top, bot = frame_rays(R, W)
    tv = sample_parameters_on(torch.device(DEV), S, eval_mode=True, include_end_pt=True)
    delta = 1.9 / (S - 1)
    sun, sky, cls = group_inputs(net, TIMES[:3])
    a, b = launch(net, top, bot, tv, delta, sun, sky, cls, 6), launch(net, top, bot, tv, delta, sun, sky, cls, 6)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert torch.equal(a[:36], launch(net, top[:36].contiguous(), bot[:36].contiguous(), tv, delta, sun, sky, cls, 6))
    t9, b9 = top[-9:].contiguous(), bot[-9:].contiguous()
    rho, col_raw, vis, adj, oob = per_sample(net, t9, b9, tv, sun)
    dl = torch.where(oob, torch.zeros(9, S), torch.full((9, S), delta))
    check_sixteen("frame_walk", f"W{W} tail", a[-9:], (rho, col_raw, vis, adj), sky, cls, dl)


@pytest.mark.parametrize("W", [64, 256, 512])
def test_early_out(golden_dir, W):
    """The opaque column of test_gpu_surface.py::test_early_out, eight copies in front of 195 other rays: the first workgroups vote themselves saturated
    and skip the third pass - the depth walked is smaller than without the early-out and greater than 18.  Behind optical depth 18 the PS left on a ray
    sum to less than exp(-18), and shade, colour and vis lie in [0, 1]: colours, sum PS and sum PS vis move by at most exp(-18) + 4 * 2^-24, sum PS s by
    (S - 1) times that."""
    from season_nerf_amd.network import _ops
    S = 96
    sd = weights(golden_dir, f"sharp_W{W}")
    ctop, cbot = lattice((8, 8))
    tv_c = torch.linspace(0, 1, S + 1)[:-1].float()
    y = oracle_density(sd, ctop, cbot, tv_c).double() * (2.0 / S)
    front, rest = y[:, :64].sum(1), y[:, 64:].sum(1)
    assert int((front > 25).sum()) >= 1
    col = int(torch.argmax(torch.where(front > 25, rest, torch.full_like(rest, -1.0))))
    net = net_of(golden_dir, f"sharp_W{W}")
    otop, obot, _ = rays(195, S, 7)
    top = torch.cat([ctop[col:col + 1].expand(8, 3).to(DEV), otop]).contiguous()
    bot = torch.cat([cbot[col:col + 1].expand(8, 3).to(DEV), obot]).contiguous()
    sun, sky, cls = group_inputs(net, TIMES[:3])
    a = (net.device_model(), top, bot, tv_c.to(DEV), 2.0 / S, sun, sky, cls)
    early, full = _ops().frame_walk(*a, 0).double().cpu(), _ops().frame_walk(*a, 4).double().cpu()
    print(f"  W={W} column {col}: carry of rays 0..7: {early[:8, 14].tolist()} with the early-out, {full[:8, 14].tolist()} without")
    assert bool((early[:8, 14] < full[:8, 14]).all()), "no pass was skipped"
    assert bool((early[:8, 14] > 18).all())
    bound = np.exp(-18.0) + 4 * EPS
    d = (early - full).abs()
    print(f"  early-out moved: rgb {float(d[:, :12].max()):.2e} acc {float(d[:, 12].max()):.2e} mi {float(d[:, 13].max()):.2e} psv {float(d[:, 15].max()):.2e}; "
          f"rays with passes skipped {int((early[:, 14] < full[:, 14]).sum())} of {top.shape[0]}")
    assert float(d[:, :12].max()) <= bound and float(d[:, 12].max()) <= bound and float(d[:, 15].max()) <= bound and float(d[:, 13].max()) <= bound * (S - 1)
    assert bool((early[:, 9:12] == 0).all())


@pytest.mark.parametrize("W", [64, 256, 512])
def test_seasons_of_one_launch_equal_single_launches(golden_dir, W):
    """One launch with T seasons against T launches with one: bit-identical rows."""
    from season_nerf_amd.network import _ops
    from season_nerf_amd.evaluator import sample_parameters_on
    net = net_of(golden_dir, f"sharp_W{W}")
    S = 40
    top, bot = frame_rays(37, W + 1)
    tv = sample_parameters_on(torch.device(DEV), S, eval_mode=True, include_end_pt=True)
    sun, sky, cls = group_inputs(net, TIMES[:MAX_T])
    a = (net.device_model(), top, bot, tv, 1.9 / (S - 1), sun, sky)
    for flags in (2, 6):
        many = _ops().frame_walk(*a, cls, flags)
        for k in range(MAX_T):
            one = _ops().frame_walk(*a, cls[k:k + 1].contiguous(), flags)
            assert torch.equal(one[:, :3], many[:, 3 * k:3 * k + 3]) and torch.equal(one[:, 12:], many[:, 12:]) and bool((one[:, 3:12] == 0).all()), (flags, k)


# ------------------------------------------------------------------------------------------------ against the reference's recorded frames
def _frame_rays_f64(g, f):
    import season_nerf_amd as sn
    return sn.sample_rays_projective(*frame_params(g, f))


def per_sample_frame(net, g, f):
    """The per-sample path on what the walk is given - the fixture's float32 end planes: `forward_seperate` on the points top (1 - t) + bot t formed in
    float32, the sums in float64 with the frame's float64 delta -> images [3,H,W,3], HM [H,W] (numpy float64)."""
    from season_nerf_amd.evaluator import sample_parameters_on
    H, W, S = (int(v) for v in g[f"f{f}_size"])
    top, bot = torch.tensor(g[f"f{f}_top"], device=DEV).reshape(-1, 3), torch.tensor(g[f"f{f}_bot"], device=DEV).reshape(-1, 3)
    tv = sample_parameters_on(torch.device(DEV), S, eval_mode=True, include_end_pt=True)
    sun, sky, cls = group_inputs(net, g["times"])
    assert np.array_equal(sun.cpu().numpy(), g["sun"].astype(np.float32))
    rho, col_raw, vis, adj, oob = per_sample(net, top, bot, tv, sun)
    dl = torch.where(oob, torch.zeros(1, dtype=torch.float64), torch.full((H * W, S), float(g[f"f{f}_delta"]), dtype=torch.float64))
    rows = statement(rho.double(), col_raw.double(), vis.double(), adj.double(), sky.double().cpu(), cls.double().cpu(), dl).numpy()
    return rows[:, :9].reshape(H, W, 3, 3).transpose(2, 0, 1, 3), (2.0 * rows[:, 13] / (S - 1)).reshape(H, W)


def test_per_sample_deviation(golden_dir):
    """The measurement behind E_FRAME of test_frame_host.py: the per-sample path - the parent's kernels, which the walk does not run: `forward_seperate`
    on the same float32 points the walk forms from the fixture's end planes, float64 sums - against the recorded images and HM, over the whole fixture.
    Printed beside it: the same through `get_Img.eval_rays` on the reference's own points (its float64 lattice cast to float32)."""
    import season_nerf_amd as sn
    g = fixture(golden_dir)
    for tag in TAGS:
        net = net_of(golden_dir, tag)
        cam = sn.get_Img(net, DEV)
        e_img = e_hm = o_img = o_hm = 0.0
        for f in range(3):
            imgs, hm = per_sample_frame(net, g, f)
            e_img, e_hm = max(e_img, np.abs(imgs - g[f"{tag}_f{f}_Imgs"]).max()), max(e_hm, np.abs(hm - g[f"{tag}_f{f}_HM"]).max())
            R, delta = _frame_rays_f64(g, f)
            for k, t in enumerate(g["times"]):
                img, ps = cam.eval_rays(R, g["sun"], t, delta=delta)
                o_img = max(o_img, np.abs(img - g[f"{tag}_f{f}_Imgs"][k]).max())
            o_hm = max(o_hm, np.abs((ps[..., 0] * np.linspace(0, 2, R.shape[2]).reshape(1, 1, -1)).sum(2) - g[f"{tag}_f{f}_HM"]).max())
        print(f"  E_frame[{tag}] = (images {e_img:.4e}, HM {e_hm:.4e})   recorded: {E_FRAME[tag]}   on the reference's own points: ({o_img:.4e}, {o_hm:.4e})")
        assert e_img <= E_FRAME[tag][0] and e_hm <= E_FRAME[tag][1], "the recorded maxima no longer bound the per-sample path's deviation"


@pytest.mark.parametrize("tag", TAGS)
def test_eval_rays_vs_reference(golden_dir, tag):
    """`get_Img.eval_rays` runs the per-sample kernels on the reference's own points: image, PS and the HM formed from PS against the fixture, held to
    the measured rule on the reference's own error, 4 * (E_ref + 2^-24 * scale), E_ref = max |reference - CPU oracle in float64| over the set's frames."""
    import season_nerf_amd as sn
    g = fixture(golden_dir)
    cam = sn.get_Img(net_of(golden_dir, tag), DEV)
    e_ref = {"Imgs": 0.0, "HM": 0.0, "PS": 0.0}
    for f in range(3):
        H, W, S = (int(v) for v in g[f"f{f}_size"])
        i64, h64, p64 = direct_composite(*oracle_per_sample(golden_dir, g, tag, f, torch.float64), float(g[f"f{f}_delta"]))
        for name, o in (("Imgs", i64.reshape(3, H, W, 3)), ("HM", h64.reshape(H, W)), ("PS", p64.reshape(H, W, S))):
            e_ref[name] = max(e_ref[name], np.abs(g[f"{tag}_f{f}_{name}"] - o).max())
    for f in range(3):
        R, delta = _frame_rays_f64(g, f)
        S = R.shape[2]
        for k, t in enumerate(g["times"]):
            img, ps = cam.eval_rays(R, g["sun"], t, delta=delta)
            assert img.shape == R.shape[:2] + (3,) and ps.shape == R.shape[:3] + (1,) and img.dtype == np.float64 and ps.dtype == np.float64
            d = np.abs(img - g[f"{tag}_f{f}_Imgs"][k]).max()
            assert d <= 4 * (e_ref["Imgs"] + EPS), (f, k, d, e_ref)
        hm = (ps[..., 0] * np.linspace(0, 2, S).reshape(1, 1, -1)).sum(2)
        d_h, d_p = np.abs(hm - g[f"{tag}_f{f}_HM"]).max(), np.abs(ps[..., 0] - g[f"{tag}_f{f}_PS"]).max()
        print(f"  {tag} frame {f}: HM {d_h:.3e} (4 (E_ref + 2 eps) = {4 * (e_ref['HM'] + 2 * EPS):.3e})   PS {d_p:.3e} ({4 * (e_ref['PS'] + EPS):.3e})")
        assert d_h <= 4 * (e_ref["HM"] + 2 * EPS) and d_p <= 4 * (e_ref["PS"] + EPS), (f, d_h, d_p, e_ref)


@pytest.mark.parametrize("tag", TAGS)
def test_walk_vs_reference(golden_dir, tag):
    """The fixture's end planes through the kernel against the reference's images and HM, all four sets and three frames: within
    2 E_FRAME[tag] + 4 * 2^-24 * scale (scale 1 for the images, 2 for HM)."""
    import season_nerf_amd as sn
    g = fixture(golden_dir)
    net = net_of(golden_dir, tag)
    assert net.resolved_precision == "bf16x3"
    for f in range(3):
        H, W, S = (int(v) for v in g[f"f{f}_size"])
        top, bot = torch.tensor(g[f"f{f}_top"], device=DEV), torch.tensor(g[f"f{f}_bot"], device=DEV)
        fw = sn.frame_walk(net, top, bot, S, float(g[f"f{f}_delta"]), g["sun"], times=g["times"])
        assert fw.rows[0].dtype == torch.float32 and fw.n_times == 3 and fw.n_rays == H * W
        imgs, hm = fw.images((H, W)).cpu().numpy(), fw.height_map((H, W)).cpu().numpy()
        d_i, d_h = np.abs(imgs - g[f"{tag}_f{f}_Imgs"]).max(), np.abs(hm - g[f"{tag}_f{f}_HM"]).max()
        print(f"  {tag} frame {f}: max |Imgs - ref| {d_i:.3e} (bound {2 * E_FRAME[tag][0] + 4 * EPS:.3e})   max |HM - ref| {d_h:.3e} (bound {2 * E_FRAME[tag][1] + 8 * EPS:.3e})")
        assert d_i <= 2 * E_FRAME[tag][0] + 4 * EPS and d_h <= 2 * E_FRAME[tag][1] + 8 * EPS


@pytest.mark.parametrize("tag", ["init_W64_s2", "sharp_W256"])
def test_get_Img_vs_reference(golden_dir, tag):
    """capture_frame, capture_frame_advanced and eval_rays_advanced under the reference's names against the fixture."""
    import season_nerf_amd as sn
    g = fixture(golden_dir)
    cam = sn.get_Img(net_of(golden_dir, tag), DEV, max_batch_size=1 << 16, per_img_tqdm=False)
    bi, bh = 2 * E_FRAME[tag][0] + 4 * EPS, 2 * E_FRAME[tag][1] + 8 * EPS
    for f in (0, 2):
        par = frame_params(g, f)
        imgs, hm = cam.capture_frame_advanced(*par, g["sun"], g["times"])
        assert isinstance(imgs, list) and len(imgs) == 3 and imgs[0].dtype == np.float64 and hm.shape == par[4][:2]
        assert np.abs(np.stack(imgs) - g[f"{tag}_f{f}_Imgs"]).max() <= bi and np.abs(hm - g[f"{tag}_f{f}_HM"]).max() <= bh
        img = cam.capture_frame(*par, g["sun"], float(g["times"][1]))
        assert img.shape == par[4][:2] + (3,) and np.array_equal(img, imgs[1])
        R, delta = _frame_rays_f64(g, f)
        imgs2, hm2 = cam.eval_rays_advanced(R, g["sun"], g["times"], delta=delta)
        assert np.array_equal(np.stack(imgs2), np.stack(imgs)) and np.array_equal(hm2, hm)


def test_more_seasons_than_a_launch_holds(golden_dir):
    """Seven seasons go in two launches: each image equals that season's own single-season walk bit for bit, and the ray statistics are the first launch's."""
    import season_nerf_amd as sn
    g = fixture(golden_dir)
    net = net_of(golden_dir, "sharp_W64")
    H, W, S = (int(v) for v in g["f0_size"])
    top, bot = torch.tensor(g["f0_top"], device=DEV), torch.tensor(g["f0_bot"], device=DEV)
    fw = sn.frame_walk(net, top, bot, S, float(g["f0_delta"]), g["sun"], times=TIMES)
    assert len(fw.rows) == 2 and fw.images((H, W)).shape == (7, H, W, 3) and bool((fw.rows[1][:, 9:12] == 0).all())
    for k, t in enumerate(TIMES):
        one = sn.frame_walk(net, top, bot, S, float(g["f0_delta"]), g["sun"], times=[t])
        assert torch.equal(one.images((H, W))[0], fw.images((H, W))[k]), k
        assert torch.equal(one.height_map((H, W)), fw.height_map((H, W)))
    cv = net.get_class_only(torch.tensor(np.stack([sn.encode_time(t) for t in TIMES[:2]]), dtype=torch.float32, device=DEV))
    by_vec = sn.frame_walk(net, top, bot, S, float(g["f0_delta"]), g["sun"], class_vecs=cv)
    assert torch.equal(by_vec.images((H, W)), fw.images((H, W))[:2])
    with pytest.raises(ValueError, match="frame_walk"):
        sn.frame_walk(net, top, bot, S, float(g["f0_delta"]), g["sun"])
    with pytest.raises(ValueError, match="frame_walk"):
        sn.frame_walk(net, top, bot, 1, float(g["f0_delta"]), g["sun"], times=[0.1])


def test_fallback_valid_range(golden_dir):
    """A valid range other than the cube goes by the float64 fallback.  (a) On frame 1, whose samples all lie inside the cube, a range that contains the
    cube changes nothing: the walk's rows against the fallback's - the float64 sums of the model's own per-sample outputs - by the kernel tests' rule.
    (b) A range smaller than the cube on frame 0 against the CPU oracle in float64 with that range, within the walk's band 2 E_FRAME + 4 * 2^-24 * scale."""
    import season_nerf_amd as sn
    from season_nerf_amd.evaluator import sample_parameters_on
    tag = "sharp_W64"
    g = fixture(golden_dir)
    net = net_of(golden_dir, tag)
    H, W, S = (int(v) for v in g["f1_size"])
    top, bot = torch.tensor(g["f1_top"], device=DEV).reshape(-1, 3), torch.tensor(g["f1_bot"], device=DEV).reshape(-1, 3)
    delta = float(g["f1_delta"])
    walk = sn.frame_walk(net, top, bot, S, delta, g["sun"], times=g["times"], early_out=False)
    wide = sn.frame_walk(net, top, bot, S, delta, g["sun"], times=g["times"], valid_range=np.array([[-1, 1.], [-1, 1], [-1, 2]]))
    assert walk.rows[0].dtype == torch.float32 and wide.rows[0].dtype == torch.float64
    tv = sample_parameters_on(torch.device(DEV), S, eval_mode=True, include_end_pt=True)
    sun, sky, cls = group_inputs(net, g["times"])
    rho, col_raw, vis, adj, oob = per_sample(net, top, bot, tv, sun)
    assert not bool(oob.any())
    dl = torch.full((H * W, S), delta, dtype=torch.float32)      # the kernel takes delta as a float, the fallback keeps the float64 one
    ref64 = statement(rho.double(), col_raw.double(), vis.double(), adj.double(), sky.double().cpu(), cls.double().cpu(), torch.full((H * W, S), delta, dtype=torch.float64))
    np.testing.assert_allclose(wide.rows[0].cpu().numpy(), ref64.numpy(), rtol=1e-12, atol=1e-12)
    check_sixteen("frame_walk", "vs fallback", walk.rows[0], (rho, col_raw, vis, adj), sky, cls, dl)
    # (b)
    vr = np.array([[-0.8, 0.8], [-0.7, 0.9], [-1.0, 0.6]])
    H, W, S = (int(v) for v in g["f0_size"])
    cam = sn.get_Img(net, DEV, valid_range=vr)
    imgs, hm = cam.capture_frame_advanced(*frame_params(g, 0), g["sun"], g["times"])
    rho, col_raw, vis, adj, sky64, cls64, _ = oracle_per_sample(golden_dir, g, tag, 0, torch.float64)
    p = _frame_rays_f64(g, 0)[0].astype(np.float32).astype(np.float64).reshape(H * W, S, 3)
    outside = ((p < vr[:, 0]) | (p > vr[:, 1])).any(-1)
    assert outside.mean() > 0.3
    i64, h64, _ = direct_composite(rho, col_raw, vis, adj, sky64, cls64, outside, float(g["f0_delta"]))
    d_i, d_h = np.abs(np.stack(imgs) - i64.reshape(3, H, W, 3)).max(), np.abs(hm - h64.reshape(H, W)).max()
    print(f"  valid range smaller than the cube: max |Imgs - float64 oracle| {d_i:.3e}   max |HM - float64 oracle| {d_h:.3e}")
    assert d_i <= 2 * E_FRAME[tag][0] + 4 * EPS and d_h <= 2 * E_FRAME[tag][1] + 8 * EPS
    cube = sn.get_Img(net, DEV).capture_frame_advanced(*frame_params(g, 0), g["sun"], g["times"])
    assert np.abs(np.stack(cube[0]) - np.stack(imgs)).max() > 1e-3, "the smaller range changed nothing"


def test_fallback_int8(golden_dir):
    """An int8-resolved network is not served by the kernels: the float64 fallback on its own per-sample outputs.  Against the reference's recorded
    frames at the project's band for int8 digits on the init-law set (rtol 5e-5, atol 5e-5: test_gpu_surface.py), and against the bf16x3 walk of the
    same weights within that band plus the walk's own."""
    import season_nerf_amd as sn
    from season_nerf_amd import render as R_
    tag = "init_W64_s2"
    g = fixture(golden_dir)
    net8, net = net_of(golden_dir, tag, "i8x3"), net_of(golden_dir, tag)
    assert net8.resolved_precision == "i8x3" and not R_._walks(net8)
    for f in range(3):
        H, W, S = (int(v) for v in g[f"f{f}_size"])
        top, bot = torch.tensor(g[f"f{f}_top"], device=DEV), torch.tensor(g[f"f{f}_bot"], device=DEV)
        a = (top, bot, S, float(g[f"f{f}_delta"]), g["sun"])
        fb, walk = sn.frame_walk(net8, *a, times=g["times"]), sn.frame_walk(net, *a, times=g["times"])
        assert fb.rows[0].dtype == torch.float64
        imgs, hm = fb.images((H, W)).cpu().numpy(), fb.height_map((H, W)).cpu().numpy()
        np.testing.assert_allclose(imgs, g[f"{tag}_f{f}_Imgs"], rtol=5e-5, atol=5e-5)
        np.testing.assert_allclose(hm, g[f"{tag}_f{f}_HM"], rtol=5e-5, atol=5e-5)
        np.testing.assert_allclose(imgs, walk.images((H, W)).cpu().numpy(), rtol=5e-5, atol=5e-5 + 2 * E_FRAME[tag][0] + 4 * EPS)
        np.testing.assert_allclose(hm, walk.height_map((H, W)).cpu().numpy(), rtol=5e-5, atol=5e-5 + 2 * E_FRAME[tag][1] + 8 * EPS)


def test_op(golden_dir):
    """opcheck (schema and fake kernel), argument errors, a NULL model, and two launches bit for bit."""
    import season_nerf_amd as sn
    from season_nerf_amd.evaluator import sample_parameters_on
    ops = sn.ops.load()
    net = net_of(golden_dir, "sharp_W64")
    h = net.device_model()
    top, bot = frame_rays(37, 1)
    tv = sample_parameters_on(torch.device(DEV), 40, eval_mode=True, include_end_pt=True)
    sun, sky, cls = group_inputs(net, TIMES[:3])
    a = ops.frame_walk(h, top, bot, tv, 0.05, sun, sky, cls, 2)
    b = ops.frame_walk(h, top, bot, tv, 0.05, sun, sky, cls, 2)
    assert a.shape == (37, 16) and a.dtype == torch.float32 and a.device == top.device and torch.equal(a, b)
    assert ops.frame_walk(h, top[:0], bot[:0], tv, 0.05, sun, sky, cls, 0).shape == (0, 16)
    torch.library.opcheck(torch.ops.season_nerf.frame_walk.default, (h, top, bot, tv, 0.05, sun, sky, cls, 2), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(RuntimeError, match="top"):
        ops.frame_walk(h, top[:, :2].contiguous(), bot, tv, 0.05, sun, sky, cls, 0)
    with pytest.raises(RuntimeError, match="bot"):
        ops.frame_walk(h, top, bot[:5], tv, 0.05, sun, sky, cls, 0)
    with pytest.raises(RuntimeError, match="float32"):
        ops.frame_walk(h, top.double(), bot, tv, 0.05, sun, sky, cls, 0)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.frame_walk(h, top, bot, tv, 0.05, sun.cpu(), sky, cls, 0)
    with pytest.raises(RuntimeError, match="tvals"):
        ops.frame_walk(h, top, bot, tv[:1], 0.05, sun, sky, cls, 0)
    with pytest.raises(RuntimeError, match="sun and sky"):
        ops.frame_walk(h, top, bot, tv, 0.05, sun, sky.reshape(1, 3), cls, 0)
    with pytest.raises(RuntimeError, match="class_vecs"):
        ops.frame_walk(h, top, bot, tv, 0.05, sun, sky, torch.cat([cls, cls])[:MAX_T + 1].contiguous(), 0)
    with pytest.raises(RuntimeError, match="delta"):
        ops.frame_walk(h, top, bot, tv, 0.0, sun, sky, cls, 0)
    with pytest.raises(RuntimeError, match="delta"):
        ops.frame_walk(h, top, bot, tv, float("nan"), sun, sky, cls, 0)
    with pytest.raises(RuntimeError, match="flags"):
        ops.frame_walk(h, top, bot, tv, 0.05, sun, sky, cls, 1)
    with pytest.raises(RuntimeError, match="NULL"):
        ops.frame_walk(0, top, bot, tv, 0.05, sun, sky, cls, 0)
    net8 = net_of(golden_dir, "init_W64_s2", "i8x3")
    with pytest.raises(RuntimeError, match="snerf_field_frame_walk"):
        ops.frame_walk(net8.device_model(), top, bot, tv, 0.05, sun, sky, cls, 0)
