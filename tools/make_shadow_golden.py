#!/usr/bin/env python
"""Generate tests/golden/shadow_points.npz by running the REFERENCE itself: `eval_shadow_data` and `shadow_anaylysis`
(T_NeRF_Eval_Utils/mg_Shadow_Eval.py:72-104,134-163) for five sun directions over a 6 x 6 lattice of ground points, at 96 and at 40 samples per ray,
for four weight sets.  Modelled on tools/make_height_golden.py: the reference imports, stubs and weight set-up of tools/make_golden.py and the
`sharp_state` recipe of make_height_golden are reused; nothing of the reference is copied.  Needs a CPU and the reference checkout only.

    python tools/make_shadow_golden.py

What is stored:
    tags, Z_list, world_center_LLA, W2L_H, shadow_angles [M,2] (el, az in degrees), ground_points [G,2], sun_vecs [M,3] (world_angle_2_local_vec)
    per weight set `tag` and Z:
      {tag}_Z{Z}_Exact_Vis [M,G,Z] float32      get_PV along the sun ray (the reference computes it in fp32; its float64 array holds these values)
      {tag}_Z{Z}_Est_Vis   [M,G,Z] float32      the learned solar visibility
      {tag}_Z{Z}_Sky_Col   [M,3]   float64
      {tag}_Z{Z}_scores    [8]     float64      shadow_anaylysis: the order of `score_keys`
Weight sets: init_W64_s2 (the init law, seed 2) and sharp_W64 / sharp_W256 / sharp_W512, as in tools/make_height_golden.py.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg      # noqa: E402  (stubs the reference's optional imports and puts it on sys.path)
from make_height_golden import sharp_state      # noqa: E402
from T_NeRF_Eval_Utils.mg_Shadow_Eval import eval_shadow_data, shadow_anaylysis      # noqa: E402

ANGLES = np.array([[75.0, 20.0], [40.0, 140.0], [20.0, 250.0], [55.0, 310.0], [88.0, 0.0]])
Z_LIST = (96, 40)
KEYS = ("Acc", "Prec_Sun", "Recall_Sun", "Prec_Shadow", "Recall_Shadow", "Loss", "Avg_Error", "Avg_Offset")


def main():
    lin = np.linspace(-1, 1, 6)
    ground = np.array([(x, y) for x in lin for y in lin])
    out = {"tags": np.array(["init_W64_s2", "sharp_W64", "sharp_W256", "sharp_W512"]), "Z_list": np.array(Z_LIST), "world_center_LLA": mg.WC,
           "W2L_H": mg.H4, "shadow_angles": ANGLES, "ground_points": ground, "score_keys": np.array(KEYS),
           "sun_vecs": np.array([mg.world_angle_2_local_vec(a[0], a[1], mg.WC, mg.H4) for a in ANGLES], dtype=np.float64)}
    nets = {"init_W64_s2": mg.make_net(64, 4, 2)[0]}
    for W in (64, 256, 512):
        net = mg.T_NeRF(W, 4)
        r = net.load_state_dict(sharp_state(W), strict=True)
        assert not r.missing_keys and not r.unexpected_keys
        nets[f"sharp_W{W}"] = net
    for tag, net in nets.items():
        net.eval()
        for Z in Z_LIST:
            ex, est, sky = eval_shadow_data(net, ANGLES, ground, Z, mg.WC, mg.H4, 15000, torch.device("cpu"))
            sc = shadow_anaylysis(ground, ANGLES, {"Exact_Vis": ex, "Est_Vis": est, "Sky_Col": sky})
            ex32, est32 = ex[..., 0].astype(np.float32), est[..., 0].astype(np.float32)
            assert np.array_equal(ex32.astype(np.float64), ex[..., 0]) and np.array_equal(est32.astype(np.float64), est[..., 0])      # fp32 values: nothing lost
            out[f"{tag}_Z{Z}_Exact_Vis"], out[f"{tag}_Z{Z}_Est_Vis"], out[f"{tag}_Z{Z}_Sky_Col"] = ex32, est32, np.asarray(sky, dtype=np.float64)
            out[f"{tag}_Z{Z}_scores"] = np.array([sc[k] for k in KEYS], dtype=np.float64)
            band = (np.abs(ex32 - .5) < 1e-3) | (np.abs(est32 - .5) < 1e-3)
            print(f"{tag} Z={Z}: exact>.5 {np.mean(ex32 > .5):.3f} est>.5 {np.mean(est32 > .5):.3f} " + " ".join(f"{k}={sc[k]:.4f}" for k in KEYS)
                  + f" | band 1e-3: {band.mean() * 100:.2f} % of samples, {int(band.any(2).sum())} rays", flush=True)
    path = os.path.join(mg.OUT, "shadow_points.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
