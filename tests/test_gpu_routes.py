"""Finalized models through the C ABI's walk entry points: the refusals of the modes that have no walk kernel, and the walk stream's re-upload when the
number of suns changes.  W = 64, C = 4, 8 rays of 33 samples: two passes of 32, the second ragged."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc

pytestmark = pytest.mark.gpu
W, CN, R, S = 64, 4, 8, 33
ONLY = " for SNERF_PREC_BF16X3 at widths 64, 256 and 512 only"


def _finalized(L, precision):
    m = L.snerf_model_create(W, CN)
    assert m and L.snerf_model_set_precision(m, precision) == 0
    for k, v in orc.init_weights(W, CN, 4).items():
        if v.is_floating_point():
            a = np.ascontiguousarray(v.numpy(), dtype=np.float32)
            assert L.snerf_model_set_tensor(m, k.encode(), a.ctypes.data, a.size) == 0
    assert L.snerf_model_finalize(m) == 0, L.snerf_last_error()
    return m


def _rays():
    g = torch.Generator().manual_seed(9)
    xy = lambda: torch.rand(R, 2, generator=g) * 2 - 1
    top = torch.cat([xy(), torch.ones(R, 1)], 1).cuda()
    bot = torch.cat([xy(), -torch.ones(R, 1)], 1).cuda()
    tvals = torch.linspace(0, 1, S).cuda()
    return top, bot, tvals


@pytest.mark.parametrize("precision", [2, 1], ids=["i8x3", "bf16"])
def test_modes_without_walk_kernels_refuse_the_walks(precision):
    import season_nerf_amd as sn
    L = sn._lib.lib()
    m = _finalized(L, precision)
    top, bot, tvals = _rays()
    p = lambda t: t.data_ptr()
    sun, out = torch.full((R, 3), 0.5).cuda(), torch.zeros(R, 16).cuda()
    per = torch.zeros(R, S).cuda()
    sun3 = (C.c_double * 3)(0.3, -0.2, 0.8)
    fo = sn._lib.FieldOut()
    calls = {
        "snerf_field_sun_walk_rays: the sun walk exists": lambda: L.snerf_field_sun_walk_rays(m, R, S, p(top), p(bot), p(tvals), 2, p(sun), None, C.byref(fo), None),
        "snerf_field_ray_surface: the ray-surface kernels exist": lambda: L.snerf_field_ray_surface(m, R, S, p(top), p(bot), p(tvals), 0, p(out), None),
        "snerf_field_shadow_walk: the shadow-walk kernels exist": lambda: L.snerf_field_shadow_walk(m, R, S, p(top), p(bot), p(sun), p(tvals), 0, p(out), None),
        "snerf_field_solar_audit: the solar-audit kernels exist": lambda: L.snerf_field_solar_audit(m, R, S, p(top), p(bot), p(tvals), C.addressof(sun3), p(per), p(per),
                                                                                                   2, p(out), None, None),
        "snerf_field_frame_walk: the frame-walk kernels exist": lambda: L.snerf_field_frame_walk(m, R, S, p(top), p(bot), p(tvals), 0.05, p(sun), p(sun), 2, p(per),
                                                                                                 0, p(out), None),
    }
    for message, call in calls.items():
        assert call() == -1 and L.snerf_last_error().decode() == message + ONLY, (message, L.snerf_last_error())      # SNERF_E_INVALID
    torch.cuda.synchronize()
    L.snerf_model_destroy(m)


def test_walk_stream_follows_the_number_of_suns():
    """n_suns 2, 3, 2 on one model: every change rebuilds the device copy of the walk stream; the third result is the first, bit for bit, and the two suns
    the walks share give the same visibility in all three."""
    import season_nerf_amd as sn
    L = sn._lib.lib()
    m = _finalized(L, 0)
    top, bot, tvals = _rays()
    suns = torch.tensor([[0.3, -0.2, 0.8], [-0.5, 0.1, 0.6], [0.1, 0.7, 0.4]])
    suns = (suns / suns.norm(dim=1, keepdim=True)).cuda()
    N = R * S

    def walk(n):
        o = {"d_rho": torch.zeros(N), "d_solar_vis": torch.zeros(n, N), "d_col_raw": torch.zeros(N, 3), "d_adjust": torch.zeros(N, CN, 3), "d_points": torch.zeros(N, 3)}
        o = {k: v.cuda() for k, v in o.items()}
        fo = sn._lib.FieldOut(**{k: v.data_ptr() for k, v in o.items()})
        rc = L.snerf_field_sun_walk_rays(m, R, S, top.data_ptr(), bot.data_ptr(), tvals.data_ptr(), n, suns.data_ptr(), None, C.byref(fo), None)
        assert rc == 0, L.snerf_last_error()
        torch.cuda.synchronize()
        return o

    a, b, c = walk(2), walk(3), walk(2)
    for k in a:
        assert torch.equal(a[k], c[k]), k
        assert float(a[k].abs().max()) > 0, k
    assert torch.equal(b["d_solar_vis"][:2], a["d_solar_vis"]) and torch.equal(b["d_rho"], a["d_rho"])
    L.snerf_model_destroy(m)
