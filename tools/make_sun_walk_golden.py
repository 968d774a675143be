#!/usr/bin/env python
"""Generate tests/golden/sun_walk_W64.npz by running the REFERENCE itself: one view under several sun directions and times, rendered the way
`Full_Eval_Seasons` does (T_NeRF_Eval_Utils/mg_Season_Eval.py:74-98) - one `component_render_by_dir` per sun direction, one
`get_imgs_from_Img_Dict_t_step` per (sun, time).  Modelled on `gen_render` of tools/make_golden.py, whose reference imports, stubs and
weight set-up it reuses; nothing of the reference is copied.  Needs a CPU and the reference checkout only.

    python tools/make_sun_walk_golden.py

What is stored (init-law weights, the seed of render_W64_s2; float32 unless noted):
    view, suns [M,2], times [T], size (H, W, S), WC, H                        the inputs
    Rho, Base_Col, Adjust_col, Deltas                                         per-sample arrays, which do not depend on the sun (recorded once)
    Est_Solar_Vis [M,R,S,1], Sky_Col0 [M,3] (float64)                         per sun, from the reference's own dict
    classes [T,C]                                                             get_class_only of the times
    imgs [M,T,H,W,3] (float64)                                                get_imgs_from_Img_Dict_t_step per sun with those class vectors
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg      # noqa: E402  (stubs the reference's optional imports and puts it on sys.path)

VIEW = (70, 20)
SUNS = [(30, 90), (45, 120), (60, 200), (20, 300), (75, 10)]
TIMES = [0.1, 0.45, 0.8]
SIZE = (6, 7, 40)
W, SEED = 64, 2


def main():
    net, _ = mg.make_net(W, 4, SEED)
    out = {"W": W, "C": 4, "seed": SEED, "WC": mg.WC, "H": mg.H4, "view": np.array(VIEW, dtype=np.float64), "suns": np.array(SUNS, dtype=np.float64),
           "times": np.array(TIMES, dtype=np.float64), "size": np.array(SIZE)}
    with torch.no_grad():
        cls = net.get_class_only(torch.tensor(np.stack([mg.encode_time(t) for t in TIMES]), dtype=torch.float32)).numpy()
    out["classes"] = cls
    sv, sky, imgs = [], [], []
    for j, sun in enumerate(SUNS):
        d = mg.component_render_by_dir(net, VIEW, sun, TIMES[0], SIZE, mg.WC, mg.H4, torch.device("cpu"), include_exact_solar=False)
        if j == 0:
            for k in ["Rho", "Base_Col", "Adjust_col", "Deltas"]:
                out[k] = mg.f32(d[k])
        else:      # the premise of the walk: nothing but the solar branch and the sky colour depends on the sun
            for k in ["Rho", "Base_Col", "Adjust_col", "Deltas"]:
                assert np.array_equal(out[k], mg.f32(d[k])), k
        sv.append(mg.f32(d["Est_Solar_Vis"]))
        sky.append(np.asarray(d["Sky_Col"][0, 0], dtype=np.float64))
        imgs.append(mg.get_imgs_from_Img_Dict_t_step(d, SIZE, cls.astype(np.float64)))
    out["Est_Solar_Vis"], out["Sky_Col0"], out["imgs"] = np.stack(sv), np.stack(sky), np.stack(imgs)
    path = os.path.join(mg.OUT, "sun_walk_W64.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
