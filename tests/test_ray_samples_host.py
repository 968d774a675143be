"""CPU-only check of `render._ray_samples`, the one copy of the sample points and deltas the layer-wise walks form: it is the four torch lines it replaced."""
import torch


def test_ray_samples_are_the_four_lines():
    from season_nerf_amd.render import _ray_samples
    S = 5
    tv = torch.linspace(0, 1, S + 1)[:-1].float()
    tops = torch.tensor([[0.3, -0.2, 1.0], [-0.9, 0.7, 1.0], [1.4, 0.1, 1.0]])      # the third ray's top lies outside the cube
    bots = torch.tensor([[0.1, 0.4, -1.0], [-0.5, 0.9, -1.0], [0.2, -0.3, -1.0]])
    n = tops.shape[0]
    for zero_oob in (False, True):
        t = tv.reshape(1, S, 1)
        p = tops.unsqueeze(1) * (1.0 - t) + bots.unsqueeze(1) * t
        delta = (torch.sqrt(torch.sum((tops - bots) ** 2, 1)) / S).reshape(n, 1).expand(n, S)
        if zero_oob:
            delta = torch.where((p.abs() > 1).any(2), torch.zeros_like(delta), delta)
        got_p, got_delta = _ray_samples(tops, bots, tv, S, zero_oob)
        assert torch.equal(got_p, p) and torch.equal(got_delta, delta)
        outside = (p.abs() > 1).any(2)
        assert outside[2].any() and not outside[:2].any()                # the case is what it says
        assert bool((got_delta[outside] == 0).all()) == zero_oob
