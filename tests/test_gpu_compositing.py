"""The four wave-per-ray compositing kernels on their own - composite_kernel (snerf_composite_rays / _dt), sweep_kernel
(snerf_composite_sweep), transmittance_kernel (snerf_transmittance) and composite_bwd_kernel (through a trainer and
snerf_trainer_debug_read) - against the reference's formulas in float64 torch on the CPU (oracle.composite_arrays / sweep_arrays /
get_PV, pinned to the reference's recorded outputs by tests/test_oracle_golden.py), at every chunk edge of both lane maps and on
densities from fog to opaque surfaces (10^2 .. 10^6).

Inputs are fp32 tensors from a seeded CPU generator; the reference gets the same fp32 values cast to float64.  The segment length
is computed by the kernels in fp32: d_delta is checked against the float64 formula to 2 ulp, and the kernel's own delta (cast to
double) enters the reference for everything downstream, so that the comparison isolates the scans and the sums.

Tolerances are measured, not chosen.  For every case the same formulas are also evaluated in torch fp32 on the CPU; E_ref is the
largest deviation of that evaluation from float64 for the output in the case.  A kernel value must stay within
    FACTOR * (E_ref + 2^-24 * scale)          scale = the largest float64 magnitude of that output in the ray (1 for PV / PE / PS)
of float64, FACTOR = 4 in the forward kernels (a six-level tree plus carry against a sequential cumsum, a device expf of up to
2 ulp against the host's 1) and 8 in the backward (a second, suffix scan).  The colour outputs of the sweep, whose sigmoids run on
v_exp_f32 + v_rcp_f32 (~2e-7 relative), get the floor 1e-6 * scale instead of 4 * 2^-24 * scale.  No case is skipped or masked;
NaN is accepted only where float64 is NaN too (surf_dist of a ray with sum PS == 0).

One margin was widened after the first run on an MI355X, for every case alike.  surf_loc and surf_dist are quotients by sum PS: on a ray
that absorbs little (smooth family, flags 3, S = 2: two samples inside the cube, sum PS = 3.7e-3) the half ulp every fp32 PE = 1 - exp(-y)
carries moves them by 2^-25 sum_s PV_s |x_s - x| / sum PS whatever the implementation.  The kernel's PE on that ray was 0.56 ulp from
float64 and its surf_loc 6e-9 from the float64 quotient of its own PS, yet 4.3e-6 from float64 with E_ref = 7.0e-7 (1.5 x the
tolerance).  That term, from float64 quantities alone, is added to the floor of these two outputs; floor and term together never
exceed 1e-5 * scale.

Measured on an MI355X - E_ref of the case that came closest, and the kernels' worst deviation as a fraction of the tolerance:
    composite_kernel      smooth 0.73 (surf_loc, E_ref 7.0e-7), mixed 1.00 (shadow, E_ref 7.5e-9), surface 0.76 (shadow, 1.6e-8), wall 0.52 (rgb, 2.4e-8), prior 0.34 (shadow, 1.4e-8)
    transmittance_kernel  smooth 0.18 (5.2e-8), mixed 0.19 (5.0e-8), surface 0.20 (5.3e-8), wall 0.18 (4.8e-8), prior 0.01 (2.8e-9)
    sweep_kernel          smooth 0.69 (raw_shadow, 4.1e-8), mixed 0.78 (raw_shadow, 1.7e-8), surface 0.64 (raw_shadow, 1.8e-8), wall 0.56 (shadow_adjust, 3.4e-7),
                          prior 0.22 (shadow_adjust, 1.2e-7)
    composite_bwd_kernel  gain 1: 0.38 (d_sky, 8.7e-8), gain 300: 0.29 (d_rho, 2.2e-10), gain 3e4: 0.19 (d_rho, 2.0e-15)
With the exclusive prefix formed as `inclusive - own` (the kernels before this file existed) the surface and wall families fail in all three
forward kernels, by up to 36 000 x the tolerance, and with the suffix as `total - inclusive` the gain-300 backward by up to 15 x.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc

pytestmark = pytest.mark.gpu

S_ALL = [1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 200, 257]     # one lane, chunk edges of both lane maps, three and five chunks
R_ALL = [1, 3, 4, 5, 1027]                                             # four rays per workgroup: ragged last block
FAMILIES = ["smooth", "empty", "mixed", "surface", "wall", "prior"]
SENT, PAD = -7777.0, 3                                                 # sentinel rows behind every output
EPS = 2.0 ** -24
COMP_OUT = {"d_rgb": 3, "d_albedo": 3, "d_pv": "S", "d_pe": "S", "d_ps": "S", "d_delta": "S", "d_shadow": 1, "d_acc": 1, "d_surf_loc": 3, "d_surf_dist": 1}
SWEEP_OUT = {"d_season": "T", "d_shaded": "T", "d_base": 3, "d_shadow_adjust": 3, "d_raw_shadow": 1, "d_classic": "T"}
WORST = {}                                                             # (kernel, family, output) -> largest deviation / tolerance seen, printed per test


def _env():
    import season_nerf_amd as sn
    L = sn._lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return sn, L, st


def _gen(*seed):
    return torch.Generator(device="cpu").manual_seed(int(sum((i + 1) * 1000003 * int(s) for i, s in enumerate(seed)) % (2 ** 31)))


def _p(t):
    return t.data_ptr() if t is not None else None


# ---------------------------------------------------------------------------------------------------------------------
# inputs
def _tvals(S):
    return torch.linspace(0, 1, S + 1)[:-1].contiguous()


def _rays(R, g, oob=False, S=1):
    """Rays through the cube; with `oob` a mix that leaves it through the top, through a side, or lies outside altogether, and ray 0 the exact
    hit top = (0,0,1), bot = (0,0,-1) (its t = 0 sample is ON the face: inside).  Every other sample stays 1e-5 away from a face."""
    u = lambda n, lo, hi: torch.rand(R, n, generator=g) * (hi - lo) + lo
    top = torch.cat([u(2, -0.9, 0.9), u(1, 0.5, 0.95)], 1)
    bot = torch.cat([u(2, -0.9, 0.9), u(1, -0.95, -0.5)], 1)
    if not oob:
        return top.contiguous(), bot.contiguous()
    k = torch.arange(R) % 5
    top[k == 1, 2] = 1.6                                            # enters through the top face
    top[k == 2, 0] = 1.7                                            # enters through a side
    top[k == 3, 0] = top[k == 3, 0] + 2.5; bot[k == 3, 0] = bot[k == 3, 0] + 2.5      # never inside
    safe_t, safe_b = torch.tensor([0.3, -0.2, 0.9]), torch.tensor([-0.1, 0.4, -0.9])
    p = _points(top, bot, _tvals(S)).double()
    near = ((p.abs() - 1).abs() < 1e-5).any(2).any(1)
    top[near], bot[near] = safe_t, safe_b
    top[0], bot[0] = torch.tensor([0.0, 0.0, 1.0]), torch.tensor([0.0, 0.0, -1.0])
    return top.contiguous(), bot.contiguous()


def _points(top, bot, tv):
    """top (1 - t) + bot t in fp32 with separate multiplies and adds, as the kernels form it (__fmul_rn / __fadd_rn)."""
    t = tv.reshape(1, -1, 1)
    omt = 1.0 - t
    return top.unsqueeze(1) * omt + bot.unsqueeze(1) * t


def _ray_delta64(top, bot, S):
    return torch.sqrt(((top.double() - bot.double()) ** 2).sum(1)) / S


def _density(family, R, S, g, delta, variant=0, edges=(63, 64, 127, 128)):
    """[R,S] fp32 densities.  delta: [R] or [R,S] fp32 segment lengths (the prior family is 4.6 / delta); `variant` rotates the surface positions over
    the rays so that a one-ray batch meets every position as S varies."""
    smooth = torch.nn.functional.softplus(3 * torch.randn(R, S, generator=g))
    s_idx = torch.arange(S).reshape(1, S)
    big = 10 ** (torch.rand(R, S, generator=g) * 4 + 2)
    rnd = torch.randint(0, S, (R, 1), generator=g)
    if family == "smooth":
        return smooth
    if family == "empty":
        return torch.zeros(R, S)
    if family == "mixed":                                           # ray 1 of every block of four is empty: its three neighbours are not
        rho = smooth.clone()
        rho[torch.arange(R) % 4 == 1] = 0.0
        return rho
    if family == "surface":
        haze = torch.rand(R, S, generator=g) * 3
        spots = [0, S - 1] + [e for e in edges if e < S] + [-1]
        pos = torch.tensor([spots[(r + variant) % len(spots)] for r in range(R)]).reshape(R, 1)
        pos = torch.where(pos < 0, rnd, pos)
        return torch.where(s_idx == pos, big, haze)
    if family == "wall":
        return torch.where(s_idx >= rnd, big, torch.rand(R, S, generator=g) * 3)
    if family == "prior":
        d = delta if delta.dim() == 2 else delta.reshape(R, 1).expand(R, S)
        d = torch.where(d > 0, d, torch.ones_like(d))
        return torch.where(s_idx >= rnd, -torch.log(torch.tensor(1 - 0.99)) / d, torch.zeros(R, S))
    raise ValueError(family)


# ---------------------------------------------------------------------------------------------------------------------
# comparison
def _check(kernel, family, name, got, ref64, ref32, factor=4, floor=EPS, unit_scale=False, rounding=None):
    """got (fp32, from the GPU), ref64, ref32: same shape [R, ...]; scale per ray = max |ref64| over the ray's entries of this output.
    rounding (optional, same shape): what half an ulp on every PE moves this output by (the quotients surf_loc / surf_dist); added to the floor, the two
    together capped at 1e-5 * scale."""
    got, ref32 = got.double(), ref32.double()
    R = ref64.shape[0]
    nan = torch.isnan(ref64)
    assert torch.equal(torch.isnan(got), nan), f"{kernel}/{family}/{name}: NaN positions differ from float64"
    assert torch.equal(torch.isnan(ref32), nan), f"{kernel}/{family}/{name}: the fp32 evaluation is NaN elsewhere than float64"
    assert bool(torch.isfinite(got[~nan]).all()), f"{kernel}/{family}/{name}: non-finite value"
    z = torch.zeros_like(ref64)
    e_ref = float(torch.where(nan, z, (ref32 - ref64).abs()).max()) if ref64.numel() else 0.0
    mag = torch.where(nan, z, ref64.abs()).reshape(R, -1).max(1).values
    if unit_scale:
        mag = torch.ones_like(mag)
    fl = (factor * floor * mag).reshape([R] + [1] * (ref64.dim() - 1))
    if rounding is not None:
        cap = torch.maximum(fl, (1e-5 * mag).reshape(fl.shape))
        fl = torch.minimum(fl + factor * torch.nan_to_num(rounding, nan=0.0, posinf=0.0), cap)
    tol = factor * e_ref + fl
    err = torch.where(nan, z, (got - ref64).abs())
    ratio = float((err / tol.clamp_min(1e-300)).max()) if ref64.numel() else 0.0
    key = (kernel, family, name)
    if ratio >= WORST.get(key, (-1.0,))[0]:
        WORST[key] = (ratio, e_ref, float(err.max()) if err.numel() else 0.0)
    bad = err > tol
    assert not bool(bad.any()), (f"{kernel}/{family}/{name}: {int(bad.sum())} entries outside {factor} * (E_ref {e_ref:.2e} + {floor:.1e} * scale); worst deviation "
                                 f"{float(err.max()):.3e}, {ratio:.1f} x the tolerance")


def _report(kernel):
    rows = {}
    for (k, fam, name), (ratio, e_ref, err) in WORST.items():
        if k == kernel:
            cur = rows.get(fam)
            if cur is None or ratio > cur[0]:
                rows[fam] = (ratio, e_ref, err, name)
    for fam, (ratio, e_ref, err, name) in rows.items():
        print(f"  {kernel:>14} {fam:>8}: worst deviation / tolerance {ratio:.3f} ({name}: deviation {err:.2e}, E_ref {e_ref:.2e})")


def _alloc(rows, width, extra=PAD):
    return torch.full(((rows + extra) * width,), SENT, device="cuda")


# ---------------------------------------------------------------------------------------------------------------------
# snerf_composite_rays
def _composite(L, st, R, S, top, bot, tv, rho, col, sv, sky, flags, prior=None, trust=1.0, trust_dev=None, want=None):
    """-> {name: cpu tensor [R, width]} of the requested outputs (all by default); checks the sentinel rows behind each."""
    sn = __import__("season_nerf_amd")
    want = list(COMP_OUT) if want is None else want
    width = {k: (S if v == "S" else v) for k, v in COMP_OUT.items()}
    bufs = {k: _alloc(R, width[k]) for k in want}
    co = sn._lib.CompositeOut(**{k: bufs[k].data_ptr() for k in want})
    dev = [x.cuda() for x in (top, bot, tv, rho, col, sv, sky)]
    pr = prior.cuda() if prior is not None else None
    if trust_dev is not None:
        td = torch.tensor([trust_dev], dtype=torch.float32).cuda()
        rc = L.snerf_composite_rays_dt(R, S, *[d.data_ptr() for d in dev], flags, _p(pr), td.data_ptr(), C.byref(co), st)
    else:
        rc = L.snerf_composite_rays(R, S, *[d.data_ptr() for d in dev], flags, _p(pr), C.c_float(trust), C.byref(co), st)
    sn._lib.check(rc, "composite_rays")
    torch.cuda.synchronize()
    out = {}
    for k in want:
        b = bufs[k].cpu()
        assert bool((b[R * width[k]:] == SENT).all()), f"{k}: rows behind the last ray were written"
        out[k] = b[:R * width[k]].reshape(R, width[k])
    return out


def _composite_inputs(family, R, S, g, oob, variant):
    top, bot = _rays(R, g, oob, S)
    tv = _tvals(S)
    d32 = (torch.sqrt(((top - bot) ** 2).sum(1)) / S)
    rho = _density(family, R, S, g, d32, variant).contiguous()
    col = torch.rand(R, S, 3, generator=g)
    sv = torch.rand(R, S, generator=g)
    sky = torch.rand(R, 3, generator=g)
    return top, bot, tv, rho, col, sv, sky


def _composite_case(L, st, family, R, S, flags, g, variant, prior_trust=None, dt=False):
    top, bot, tv, rho, col, sv, sky = _composite_inputs(family, R, S, g, bool(flags & 2), variant)
    pts = _points(top, bot, tv)
    outside = orc.outside_cube(pts)
    # the ray's own segment length, from a plain call (no bit 1): against float64 to 2 ulp, then the kernel's value is the reference's input
    plain = _composite(L, st, R, S, top, bot, tv, rho, col, sv, sky, flags & 1, want=["d_delta"])["d_delta"]
    d64 = _ray_delta64(top, bot, S)
    assert bool((plain == plain[:, :1]).all())
    assert bool(((plain[:, 0].double() - d64).abs() <= 2 * 2.0 ** -23 * d64).all()), "d_delta: more than 2 ulp from float64"
    ray_delta = plain[:, 0]
    delta = torch.where(outside, torch.zeros(R, S), plain) if flags & 2 else plain
    prior = None
    trust = 1.0
    if prior_trust is not None:
        prior = _density("prior", R, S, g, ray_delta, variant).contiguous()
        trust = float(np.float32(prior_trust))
    out = _composite(L, st, R, S, top, bot, tv, rho, col, sv, sky, flags, prior, trust, trust_dev=trust if dt else None)
    assert torch.equal(out["d_delta"], delta), "d_delta with flags bit 1: not the ray's segment length inside the cube and 0 outside"
    if flags & 2:
        assert not bool(outside[0, 0]) if R > 0 else True                     # the exact hit: a point on the face is inside
    refs = []
    for dt_ in (torch.float64, torch.float32):
        c = lambda a: a.to(dt_)
        refs.append(orc.composite_arrays(c(rho), c(delta), c(col), c(sv), c(sky), c(pts), ray_delta=c(ray_delta), classic_solar=bool(flags & 1),
                                         rho_prior=c(prior) if prior is not None else None, trust=trust))
    merged = prior is not None
    names = {"d_rgb": "Rendered_Col_Merged" if merged else "Rendered_Col", "d_albedo": "Albedo_Color_Merged" if merged else "Albedo_Color", "d_pv": "PV", "d_pe": "PE",
             "d_ps": "PS", "d_shadow": "Shadow", "d_acc": "Acc", "d_surf_loc": "surf_loc", "d_surf_dist": "surf_dist"}
    # surf_loc and surf_dist are quotients by sum PS: on a ray that absorbs little, the unavoidable half ulp (2^-25) on each PE = 1 - exp(-y) - a number next
    # to 1 minus a number - moves them by 2^-25 sum_s PV_s |x_s - x| / sum PS, whatever the implementation.  That is part of their floor.
    r = refs[0]
    live = ((rho * delta) > 0).double()
    w = (r["PV"] * live).unsqueeze(2)
    along = ray_delta.double().reshape(R, 1) * torch.arange(1, S + 1, dtype=torch.float64).reshape(1, S)
    rounding = {"d_surf_loc": 2.0 ** -25 * (w * (pts.double() - r["surf_loc"].unsqueeze(1)).abs()).sum(1) / (r["Acc"].unsqueeze(1) + 1e-8),
                "d_surf_dist": (2.0 ** -25 * (w[..., 0] * (along - r["surf_dist"].unsqueeze(1)).abs()).sum(1) / r["Acc"]).reshape(R, 1)}
    for k, n in names.items():
        r64, r32 = refs[0][n].reshape(R, -1), refs[1][n].reshape(R, -1)
        _check("composite", family, k, out[k], r64, r32, unit_scale=k in ("d_pv", "d_pe", "d_ps"), rounding=rounding.get(k))
    if family == "mixed" and not flags & 2:
        nan_rays = torch.isnan(out["d_surf_dist"][:, 0]).nonzero().reshape(-1).tolist()
        assert nan_rays == [r for r in range(R) if r % 4 == 1]
        for r in nan_rays:
            for nb in range(r - 1, min(r + 3, R)):
                if nb != r:
                    assert all(bool(torch.isfinite(out[k][nb]).all()) for k in COMP_OUT), f"ray {nb}, block neighbour of the empty ray {r}"
    return out


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("family", FAMILIES)
def test_composite_rays(family, flags):
    """Every output of snerf_composite_out at every S, the ray counts rotating over R_ALL (1027 x 257 included), without a prior."""
    sn, L, st = _env()
    for i, S in enumerate(S_ALL):
        R = R_ALL[(i + flags + FAMILIES.index(family)) % len(R_ALL)] if S != 257 else 1027
        _composite_case(L, st, family, R, S, flags, _gen(1, S, flags, FAMILIES.index(family)), variant=i)
    _report("composite")


@pytest.mark.parametrize("classic", [0, 1])
@pytest.mark.parametrize("trust", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("family", ["smooth", "mixed", "surface", "wall"])
def test_composite_rays_with_prior(family, trust, classic):
    """d_rho_prior + trust: the merged colour and albedo (a different accumulator in the classic model), the un-merged per-sample outputs beside them;
    the trust in device memory (_dt) is bit-identical to the scalar form."""
    sn, L, st = _env()
    for i, S in enumerate(S_ALL):
        R = R_ALL[(i + classic) % len(R_ALL)]
        a = _composite_case(L, st, family, R, S, classic, _gen(2, S, classic, FAMILIES.index(family)), variant=i, prior_trust=trust)
        b = _composite_case(L, st, family, R, S, classic, _gen(2, S, classic, FAMILIES.index(family)), variant=i, prior_trust=trust, dt=True)
        for k in COMP_OUT:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k}: _dt differs from the scalar trust at S = {S}"
    _report("composite")


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
@pytest.mark.parametrize("with_prior", [False, True])
def test_composite_rays_each_output_alone(flags, with_prior):
    """NULL handling: an output requested alone is bit-identical to the same output requested with all the others."""
    sn, L, st = _env()
    for S in (33, 129):
        R = 5
        g = _gen(3, S, flags)
        top, bot, tv, rho, col, sv, sky = _composite_inputs("surface", R, S, g, bool(flags & 2), S)
        prior = _density("prior", R, S, g, torch.full((R,), 2.0 / S)).contiguous() if with_prior else None
        full = _composite(L, st, R, S, top, bot, tv, rho, col, sv, sky, flags, prior, 0.3)
        for k in COMP_OUT:
            one = _composite(L, st, R, S, top, bot, tv, rho, col, sv, sky, flags, prior, 0.3, want=[k])
            assert torch.equal(one[k].view(torch.int32), full[k].view(torch.int32)), f"{k} alone differs at S = {S}"


# ---------------------------------------------------------------------------------------------------------------------
# snerf_transmittance
@pytest.mark.parametrize("family", FAMILIES)
def test_transmittance(family):
    """Arbitrary per-sample deltas, zeros and a run of zeros across the chunk edge (samples 62 .. 66) among them."""
    sn, L, st = _env()
    for i, S in enumerate(S_ALL):
        R = R_ALL[(i + FAMILIES.index(family)) % len(R_ALL)] if S != 257 else 1027
        g = _gen(4, S, FAMILIES.index(family))
        delta = torch.rand(R, S, generator=g) * (4.0 / S)
        delta[torch.rand(R, S, generator=g) < 0.1] = 0.0
        delta[:, 62:67] = 0.0
        rho = _density(family, R, S, g, delta, i).contiguous()
        pv = _alloc(R, S)
        rho_d, delta_d = rho.cuda(), delta.cuda()
        sn._lib.check(L.snerf_transmittance(R, S, rho_d.data_ptr(), delta_d.data_ptr(), pv.data_ptr(), st), "transmittance")
        torch.cuda.synchronize()
        pv = pv.cpu()
        assert bool((pv[R * S:] == SENT).all())
        _check("transmittance", family, "pv", pv[:R * S].reshape(R, S), orc.get_PV(rho.double(), delta.double()), orc.get_PV(rho, delta), unit_scale=True)
    _report("transmittance")


# ---------------------------------------------------------------------------------------------------------------------
# snerf_composite_sweep
T_ALL = [1, 5, 6, 7, 12, 13, 25]            # chunks of 12 class vectors, split 6 / 6 between the half-waves


def _sweep(L, st, R, S, Cn, T, rho, col_raw, adjust, sv, sky, cvs, flags=0, deltas=None, rays=None, classic=True, want=None, adjust_dev=None):
    sn = __import__("season_nerf_amd")
    want = [k for k in SWEEP_OUT if classic or k != "d_classic"] if want is None else want
    rows = {k: (T * R if v == "T" else R) for k, v in SWEEP_OUT.items()}
    width = {k: (3 if v == "T" else v) for k, v in SWEEP_OUT.items()}
    bufs = {k: _alloc(rows[k], width[k]) for k in want}
    so = sn._lib.SweepOut(**{k: bufs[k].data_ptr() for k in want})
    dev = [x.cuda() for x in (rho, col_raw, adjust, sv, sky, cvs)]
    if adjust_dev is not None:
        dev[2] = adjust_dev
    dl = deltas.cuda() if deltas is not None else None
    ry = [x.cuda() for x in rays] if rays is not None else [None, None, None]
    sn._lib.check(L.snerf_composite_sweep(R, S, Cn, T, _p(ry[0]), _p(ry[1]), _p(ry[2]), _p(dl), dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(),
                                          dev[3].data_ptr(), dev[4].data_ptr(), dev[5].data_ptr(), flags, C.byref(so), st), "composite_sweep")
    torch.cuda.synchronize()
    out = {}
    for k in want:
        b = bufs[k].cpu()
        n = rows[k] * width[k]
        assert bool((b[n:] == SENT).all()), f"{k}: rows behind the last ray were written"
        out[k] = b[:n].reshape((T, R, 3) if SWEEP_OUT[k] == "T" else (R, width[k]))
    return out


def _sweep_inputs(family, R, S, Cn, T, g, variant):
    delta = torch.rand(R, S, generator=g) * (4.0 / S)
    delta[torch.rand(R, S, generator=g) < 0.05] = 0.0
    rho = _density(family, R, S, g, delta, variant, edges=(31, 32, 63, 64)).contiguous()
    col_raw = torch.randn(R, S, 3, generator=g)
    adjust = 0.5 * torch.randn(R, S, Cn, 3, generator=g)
    sv = torch.rand(R, S, generator=g)
    sky = torch.rand(3, generator=g)
    cvs = torch.softmax(2 * torch.randn(T, Cn, generator=g), 1).contiguous()
    return delta, rho, col_raw, adjust, sv, sky, cvs


SWEEP_REF = {"d_season": "season", "d_shaded": "shaded", "d_base": "base", "d_shadow_adjust": "shadow_adjust", "d_raw_shadow": "raw_shadow", "d_classic": "classic"}


@pytest.mark.parametrize("classic", [True, False])
@pytest.mark.parametrize("family", FAMILIES)
def test_composite_sweep(family, classic):
    """Every output of snerf_sweep_out on explicit per-sample deltas, at every S, the class count rotating over 1 .. 5 and the number of class vectors over
    T_ALL; both template instances (d_classic set and NULL)."""
    sn, L, st = _env()
    for i, S in enumerate(S_ALL):
        R = R_ALL[(i + FAMILIES.index(family)) % len(R_ALL)] if S != 257 else 1027
        Cn, T = 1 + (i + (0 if classic else 2)) % 5, T_ALL[(i + FAMILIES.index(family)) % len(T_ALL)]
        g = _gen(5, S, FAMILIES.index(family), classic)
        delta, rho, col_raw, adjust, sv, sky, cvs = _sweep_inputs(family, R, S, Cn, T, g, i)
        out = _sweep(L, st, R, S, Cn, T, rho, col_raw, adjust, sv, sky, cvs, deltas=delta, classic=classic)
        refs = [orc.sweep_arrays(*[a.to(dt_) for a in (rho, delta, col_raw, adjust, sv, sky, cvs)]) for dt_ in (torch.float64, torch.float32)]
        for k in out:
            r64, r32, got = refs[0][SWEEP_REF[k]], refs[1][SWEEP_REF[k]], out[k]
            if SWEEP_OUT[k] == "T":                                        # [T,R,3] -> ray-major, so that the scale is the ray's
                r64, r32, got = (a.permute(1, 0, 2).reshape(R, -1) for a in (r64, r32, got))
            colour = k in ("d_season", "d_shaded", "d_base", "d_classic")
            _check("sweep", family, k, got.reshape(R, -1), r64.reshape(R, -1), r32.reshape(R, -1), floor=1e-6 / 4 if colour else EPS)
    _report("sweep")


def test_composite_sweep_adjust_alignment():
    """C = 4: a 16-byte aligned d_adjust takes the vector loads, the same data one float further on the scalar loads - bit-identical."""
    sn, L, st = _env()
    for S, T in ((33, 7), (96, 13)):
        R, Cn = 5, 4
        delta, rho, col_raw, adjust, sv, sky, cvs = _sweep_inputs("surface", R, S, Cn, T, _gen(6, S), S)
        buf = torch.zeros(adjust.numel() + 4, device="cuda")
        assert buf.data_ptr() % 16 == 0
        outs = []
        for off in (0, 1):
            view = buf[off:off + adjust.numel()]
            view.copy_(adjust.reshape(-1))
            assert view.data_ptr() % 16 == 4 * off
            outs.append(_sweep(L, st, R, S, Cn, T, rho, col_raw, adjust, sv, sky, cvs, deltas=delta, adjust_dev=view))
        for k in outs[0]:
            assert torch.equal(outs[0][k].view(torch.int32), outs[1][k].view(torch.int32)), k


@pytest.mark.parametrize("flags", [0, 2])
def test_composite_sweep_ray_derived_deltas(flags):
    """The ray-derived segment lengths (d_top / d_bot / d_tvals, flags bit 1 zeroing them outside the cube) against explicit d_deltas holding what
    snerf_composite_rays reports for the same rays and flags (checked against float64 in test_composite_rays): bit-identical; and flags bit 1 is ignored
    when the deltas are explicit."""
    sn, L, st = _env()
    for S, T, Cn in ((31, 5, 4), (65, 12, 3), (96, 25, 4), (200, 6, 5)):
        R = 37
        g = _gen(7, S, flags)
        _, rho, col_raw, adjust, sv, sky, cvs = _sweep_inputs("surface", R, S, Cn, T, g, S)
        top, bot = _rays(R, g, bool(flags & 2), S)
        tv = _tvals(S)
        dl = _composite(L, st, R, S, top, bot, tv, rho, torch.rand(R, S, 3, generator=g), sv, torch.rand(R, 3, generator=g), flags, want=["d_delta"])["d_delta"]
        if flags & 2:
            assert bool((dl == 0).any()) and bool((dl != 0).any())
        a = _sweep(L, st, R, S, Cn, T, rho, col_raw, adjust, sv, sky, cvs, flags=flags, rays=(top, bot, tv))
        b = _sweep(L, st, R, S, Cn, T, rho, col_raw, adjust, sv, sky, cvs, flags=0, deltas=dl)
        c = _sweep(L, st, R, S, Cn, T, rho, col_raw, adjust, sv, sky, cvs, flags=2, deltas=dl, rays=(top, bot, tv))
        for k in a:
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), f"{k}: ray-derived and explicit deltas differ at S = {S}"
            assert torch.equal(c[k].view(torch.int32), b[k].view(torch.int32)), f"{k}: flags bit 1 changed a sweep on explicit deltas at S = {S}"


def test_composite_sweep_each_output_alone():
    sn, L, st = _env()
    R, S, Cn, T = 5, 65, 4, 13
    delta, rho, col_raw, adjust, sv, sky, cvs = _sweep_inputs("surface", R, S, Cn, T, _gen(8), 1)
    full = _sweep(L, st, R, S, Cn, T, rho, col_raw, adjust, sv, sky, cvs, deltas=delta)
    for k in SWEEP_OUT:
        one = _sweep(L, st, R, S, Cn, T, rho, col_raw, adjust, sv, sky, cvs, deltas=delta, want=[k])
        assert torch.equal(one[k].view(torch.int32), full[k].view(torch.int32)), f"{k} alone differs"


# ---------------------------------------------------------------------------------------------------------------------
# composite_bwd_kernel, through a trainer
SIGMA_HEAD = ("G_NeRF_net.fc10Sigma.weight", "G_NeRF_net.fc10Sigma.bias")
BWD_SHAPES = [(1, 5, 33), (4, 37, 64), (4, 5, 65), (1, 37, 130), (4, 37, 200)]       # C, R, S
GAINS = [1.0, 300.0, 3.0e4]                                                         # on the density head: fog, surfaces, walls (rho > 1e4)
_ENGINES = {}


def _engine(Cn, R, S):
    """One trainer per shape (W = 64), kept for the module; the density head's initial weights beside it."""
    key = (Cn, R, S)
    if key not in _ENGINES:
        import season_nerf_amd as sn
        from season_nerf_amd.training import TrainEngine
        net = sn.T_NeRF(64, Cn)
        net.load_state_dict(orc.init_weights(64, Cn, seed=7))
        net = net.to("cuda:0").eval()
        eng = TrainEngine(net, R, 1, S)
        base = {}
        for k in SIGMA_HEAD:
            is_buffer, off, num = eng.layout[k]                  # offsets from snerf_trainer_tensor_info
            assert not is_buffer
            base[k] = (off, num, eng.params[off:off + num].clone())
        _ENGINES[key] = (net, eng, base)
    return _ENGINES[key]


def _read(L, eng, name, n):
    import season_nerf_amd as sn
    host = torch.empty(n, dtype=torch.float32)
    sn._lib.check(L.snerf_trainer_debug_read(eng.h, name.encode(), host.data_ptr(), n), "trainer_debug_read " + name)
    return host


def _bwd_case(L, st, Cn, R, S, gain, classic, trust, dt, g, which):
    """One forward + backward; `which`: the subset of (rgb, albedo, pe, rgb_merged, albedo_merged) gradients passed (the others NULL)."""
    import season_nerf_amd as sn
    net, eng, base = _engine(Cn, R, S)
    for k, (off, num, w0) in base.items():
        eng.params[off:off + num].copy_(w0 * gain)
    top, bot = _rays(R, g)
    tv = _tvals(S)
    sun = torch.nn.functional.normalize(torch.rand(R, 3, generator=g) + 0.1, dim=1)
    tau = torch.rand(R, generator=g) * 2 * np.pi
    tim = torch.stack([torch.cos(tau), torch.sin(tau), torch.ones(R), torch.zeros(R)], 1)
    dev = [x.contiguous().cuda() for x in (top, bot, tv, sun, tim)]
    dl = torch.empty(R * S, device="cuda")
    co = sn._lib.CompositeOut(d_delta=dl.data_ptr())
    sn._lib.check(L.snerf_trainer_forward_image(eng.h, R, S, *[d.data_ptr() for d in dev], 0, classic, C.byref(co), None, None, None, st), "trainer_forward_image")
    N = R * S
    rho, col, sv, sky = _read(L, eng, "rho", N).reshape(R, S), _read(L, eng, "col", N * 3).reshape(R, S, 3), _read(L, eng, "sv", N).reshape(R, S), _read(L, eng, "sky", R * 3).reshape(R, 3)
    delta = dl.cpu().reshape(R, S)
    grads = {"rgb": torch.randn(R, 3, generator=g), "albedo": torch.randn(R, 3, generator=g), "pe": torch.randn(R, S, generator=g),
             "rgb_m": torch.randn(R, 3, generator=g), "albedo_m": torch.randn(R, 3, generator=g)}
    prior = _density("prior", R, S, g, delta[:, 0]).contiguous() if trust is not None else None
    tr = float(np.float32(trust)) if trust is not None else 1.0
    gd = {k: (v.cuda() if k in which and (prior is not None or not k.endswith("_m")) else None) for k, v in grads.items()}
    pr = prior.cuda() if prior is not None else None
    if dt:
        td = torch.tensor([tr], dtype=torch.float32).cuda()
        rc = L.snerf_trainer_backward_image_dt(eng.h, _p(gd["rgb"]), _p(gd["albedo"]), None, _p(gd["pe"]), _p(pr), td.data_ptr(), _p(gd["rgb_m"]), _p(gd["albedo_m"]), st)
    else:
        rc = L.snerf_trainer_backward_image(eng.h, _p(gd["rgb"]), _p(gd["albedo"]), None, _p(gd["pe"]), _p(pr), C.c_float(tr), _p(gd["rgb_m"]), _p(gd["albedo_m"]), st)
    sn._lib.check(rc, "trainer_backward_image")
    got = {"d_rho": _read(L, eng, "d_rho", N).reshape(R, S), "d_col": _read(L, eng, "d_col", N * 3).reshape(R, S * 3), "d_sky": _read(L, eng, "d_sky", R * 3).reshape(R, 3)}
    if classic:
        got["d_sv_raw"] = _read(L, eng, "d_sv_raw", N).reshape(R, S)
    refs = []
    for dt_ in (torch.float64, torch.float32):
        leaf = {k: v.to(dt_).requires_grad_(True) for k, v in (("rho", rho), ("col", col), ("sv", sv), ("sky", sky))}
        o = orc.composite_arrays(leaf["rho"], delta.to(dt_), leaf["col"], leaf["sv"], leaf["sky"], classic_solar=bool(classic),
                                 rho_prior=prior.to(dt_) if prior is not None else None, trust=tr)
        terms = {"rgb": "Rendered_Col", "albedo": "Albedo_Color", "pe": "PE", "rgb_m": "Rendered_Col_Merged", "albedo_m": "Albedo_Color_Merged"}
        loss = sum((grads[k].to(dt_) * o[terms[k]]).sum() for k in terms if gd[k] is not None)
        loss.backward()
        z = lambda k: leaf[k].grad if leaf[k].grad is not None else torch.zeros_like(leaf[k])
        r = {"d_rho": z("rho").detach(), "d_col": z("col").detach().reshape(R, S * 3), "d_sky": z("sky").detach()}
        if classic:
            s_ = leaf["sv"].detach()
            r["d_sv_raw"] = z("sv").detach() * s_ * (1 - s_)
        refs.append(r)
    fam = f"gain {gain:g}"
    for k in got:
        _check("composite_bwd", fam, k, got[k], refs[0][k], refs[1][k], factor=8)
    return float(rho.max())


@pytest.mark.parametrize("classic", [0, 1])
@pytest.mark.parametrize("prior", ["none", "trust0", "trust0.3", "trust1", "trust0.3_dt"])
def test_composite_backward(prior, classic):
    """d_rho, d_col, d_sky (and, classic, dL/dSolar_Vis as the pre-sigmoid gradient d_sv_raw) of composite_bwd_kernel against float64 autograd of
    sum g_rgb RGB + sum g_albedo Albedo + sum g_pe PE (+ the merged terms) over the forward's own read-back fp32 values; every gradient also alone.  The
    density head is scaled until rho exceeds 1e4 (walls), which the largest gain must reach."""
    sn, L, st = _env()
    trust = None if prior == "none" else float(prior[5:].split("_")[0])
    dt = prior.endswith("_dt")
    alone = [("rgb",), ("albedo",), ("pe",)] + ([("rgb_m",), ("albedo_m",)] if trust is not None else [])
    top_rho = 0.0
    for i, (Cn, R, S) in enumerate(BWD_SHAPES):
        for j, gain in enumerate(GAINS):
            g = _gen(9, S, classic, j)
            m = _bwd_case(L, st, Cn, R, S, gain, classic, trust, dt, g, ("rgb", "albedo", "pe", "rgb_m", "albedo_m"))
            if gain == GAINS[-1]:
                top_rho = max(top_rho, m)
                assert m > 1e4, f"gain {gain:g} left rho at {m:.3g}"
            _bwd_case(L, st, Cn, R, S, gain, classic, trust, dt, g, alone[(i + j) % len(alone)])
    print(f"  largest density read back: {top_rho:.3g}")
    _report("composite_bwd")


def test_trainer_forward_refuses_zero_outside_cube():
    """flags bit 1 (zero segment length outside the cube) has no backward: snerf_trainer_forward_image refuses it instead of handing out gradients of
    another function."""
    import season_nerf_amd as sn
    _, L, st = _env()
    Cn, R, S = BWD_SHAPES[0]
    net, eng, _ = _engine(Cn, R, S)
    g = _gen(10)
    top, bot = _rays(R, g)
    dev = [x.contiguous().cuda() for x in (top, bot, _tvals(S), torch.rand(R, 3, generator=g), torch.rand(R, 4, generator=g))]
    rgb = torch.empty(R * 3, device="cuda")
    co = sn._lib.CompositeOut(d_rgb=rgb.data_ptr())
    for flags in (2, 3):
        rc = L.snerf_trainer_forward_image(eng.h, R, S, *[d.data_ptr() for d in dev], 0, flags, C.byref(co), None, None, None, st)
        assert rc == -1 and b"bit 1" in L.snerf_last_error()             # SNERF_E_INVALID
    sn._lib.check(L.snerf_trainer_forward_image(eng.h, R, S, *[d.data_ptr() for d in dev], 0, 1, C.byref(co), None, None, None, st), "trainer_forward_image")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(rgb).all())
