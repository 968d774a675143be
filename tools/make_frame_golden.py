#!/usr/bin/env python
"""Generate tests/golden/movie_frames.npz by running the REFERENCE itself: `sample_rays_projective`, `get_Img.eval_rays_advanced` and `get_Img.eval_rays`
(T_NeRF_Eval_Utils/mg_movie_maker.py:52-70,108-187) for three film frames, one sun direction and three seasons, for four weight sets.  Modelled on
tools/make_shadow_golden.py: the reference imports, stubs and weight set-up of tools/make_golden.py and the `sharp_state` recipe of make_height_golden
are reused; nothing of the reference is copied.  Needs a CPU and the reference checkout only.

    python tools/make_frame_golden.py

What is stored:
    tags, sun [3] (unit vector), times [3] (fractions of a year), n_frames
    per frame f:  f{f}_center [3], f{f}_length [3], f{f}_angles [2] (phi, theta in degrees), f{f}_size [3] (H, W, S), f{f}_delta (float64),
                  f{f}_top, f{f}_bot [H,W,3] float32 (Rays[:, :, 0] and Rays[:, :, -1], cast as the reference casts its points)
    per weight set `tag` and frame f:
                  {tag}_f{f}_Imgs [3,H,W,3] float64 (eval_rays_advanced, one image per season), {tag}_f{f}_HM [H,W] float64,
                  {tag}_f{f}_PS [H,W,S] float64 (eval_rays of the last season)
Weight sets: init_W64_s2 (the init law, seed 2) and sharp_W64 / sharp_W256 / sharp_W512, as in tools/make_height_golden.py.

Printed per set and frame: the share of samples outside the cube, the smallest distance of a float32 sample coordinate from a cube face, opaque and
empty rays, the largest difference between the seasons' images, and the reference's own sensitivity to the rounding of its input: its images and HM
re-formed by its own network on the points top (1 - t) + bot t formed in float32 instead of its float64 lattice.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg      # noqa: E402  (stubs the reference's optional imports and puts it on sys.path)
from make_height_golden import sharp_state      # noqa: E402
from T_NeRF_Eval_Utils.mg_movie_maker import get_Img, sample_rays_projective      # noqa: E402

SUN = np.array([0.3, -0.2, 0.93])
TIMES = np.array([0.1, 0.45, 0.8])
FRAMES = (((0.1, -0.05, 0.0), (0.9, 0.8, 1.0), (12.0, 35.0), (6, 5, 40)),
          ((0.02, -0.03, 0.0), (0.9, 0.95, 0.97), (0.0, 0.0), (4, 4, 33)),
          ((-0.3, 0.4, 0.1), (0.7, 0.9, 1.2), (18.0, -120.0), (5, 7, 96)))


def fp32_points(rays):
    """The sample points a float32 walk forms from the end planes: top (1 - t) + bot t with t_s = s / (S - 1), every operation rounded to float32."""
    S = rays.shape[2]
    top, bot = torch.tensor(rays[:, :, :1], dtype=torch.float32), torch.tensor(rays[:, :, -1:], dtype=torch.float32)
    t = (torch.arange(S, dtype=torch.float32) / (S - 1)).reshape(1, 1, S, 1)
    return (top * (1.0 - t) + bot * t).numpy().astype(np.float64)


def main():
    sun = SUN / np.sqrt(np.sum(SUN ** 2))
    out = {"tags": np.array(["init_W64_s2", "sharp_W64", "sharp_W256", "sharp_W512"]), "sun": sun, "times": TIMES, "n_frames": np.array(len(FRAMES))}
    nets = {"init_W64_s2": mg.make_net(64, 4, 2)[0]}
    for W in (64, 256, 512):
        net = mg.T_NeRF(W, 4)
        r = net.load_state_dict(sharp_state(W), strict=True)
        assert not r.missing_keys and not r.unexpected_keys
        nets[f"sharp_W{W}"] = net
    rays = []
    for f, (cen, length, ang, size) in enumerate(FRAMES):
        R, delta = sample_rays_projective(np.array(cen), length, ang[0], ang[1], size)
        rays.append((R, delta))
        out[f"f{f}_center"], out[f"f{f}_length"], out[f"f{f}_angles"], out[f"f{f}_size"] = np.array(cen), np.array(length), np.array(ang), np.array(size)
        out[f"f{f}_delta"] = np.float64(delta)
        out[f"f{f}_top"], out[f"f{f}_bot"] = R[:, :, 0].astype(np.float32), R[:, :, -1].astype(np.float32)
    for tag, net in nets.items():
        net.eval()
        cam = get_Img(net, torch.device("cpu"), max_batch_size=1 << 16, per_img_tqdm=False)
        for f, (R, delta) in enumerate(rays):
            imgs, hm = cam.eval_rays_advanced(R, sun, TIMES, delta=delta)
            _, ps = cam.eval_rays(R, sun, TIMES[-1], delta=delta)
            imgs = np.stack(imgs).astype(np.float64)
            out[f"{tag}_f{f}_Imgs"], out[f"{tag}_f{f}_HM"], out[f"{tag}_f{f}_PS"] = imgs, np.asarray(hm, dtype=np.float64), np.asarray(ps[..., 0], dtype=np.float64)
            p32 = R.astype(np.float32)
            outside = (np.abs(p32) > 1).any(-1)
            face = np.abs(np.abs(p32.astype(np.float64)) - 1.0).min()
            acc = ps[..., 0].sum(2)
            imgs2, hm2 = cam.eval_rays_advanced(fp32_points(R), sun, TIMES, delta=delta)
            sens_i, sens_h = np.abs(np.stack(imgs2) - imgs).max(), np.abs(hm2 - hm).max()
            seas = max(np.abs(imgs[a] - imgs[b]).max() for a in range(3) for b in range(a))
            print(f"{tag} frame {f}: outside {outside.mean() * 100:.1f} %  nearest face {face:.2e}  opaque {int((acc > .99).sum())}/{acc.size} "
                  f"empty {int((acc < .01).sum())}  seasons differ {seas:.3g}  input-rounding sensitivity img {sens_i:.2e} HM {sens_h:.2e}", flush=True)
    path = os.path.join(mg.OUT, "movie_frames.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
