#!/usr/bin/env python
"""Generate tests/golden/height_columns.npz by running the REFERENCE itself: `Eval_funcs.gen_results` (T_NeRF_Eval_Utils/Eval_funcs.py:268-296, the
column lattice and the P_Surf of `eval_HM`, :299-319) on a 12 x 10 x 96 lattice for four weight sets.  Modelled on tools/make_sun_walk_golden.py: the
reference imports, stubs and weight set-up of tools/make_golden.py are reused; nothing of the reference is copied.  Needs a CPU and the reference
checkout only.

    python tools/make_height_golden.py

What is stored (float64), per weight set `tag` in `tags`:
    shape (H, W, n)                       the lattice
    {tag}_P_Surf_sum [H,W]                P_Surf.sum(2)
    {tag}_Est_HM [H,W]                    sum_k P_Surf linspace(1, -1, n) / sum_k P_Surf  (Eval_funcs.py:319)
Weight sets: init_W64_s2 (the init law, seed 2) and sharp_W64 / sharp_W256 / sharp_W512 (the trained fixtures with the density head scaled by the
`g` of tests/golden/sharp_W*.npz, as `sharp_net` of tests/test_gpu_render.py builds them).  The weights themselves are not stored again.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg      # noqa: E402  (stubs the reference's optional imports and puts it on sys.path)
from T_NeRF_Eval_Utils.Eval_funcs import gen_results      # noqa: E402

SHAPE = (12, 10, 96)
HEAD = ("G_NeRF_net.fc10Sigma.weight", "G_NeRF_net.fc10Sigma.bias")


def sharp_state(W):
    g = dict(np.load(os.path.join(mg.OUT, f"sharp_W{W}.npz"), allow_pickle=False))
    t = dict(np.load(os.path.join(mg.OUT, str(g["source"])), allow_pickle=False))
    return {k[3:]: torch.tensor(v) * (float(g["g"]) if k[3:] in HEAD else 1.0) for k, v in t.items() if k.startswith("sd_")}


def columns(net):
    _, _, _, P_Surf, _ = gen_results(net, SHAPE[:2], SHAPE[2], torch.device("cpu"), 4096)
    z = np.linspace(1, -1, SHAPE[2]).reshape([1, 1, -1])
    return P_Surf.sum(2), np.sum(P_Surf * z, 2) / np.sum(P_Surf, 2)


def main():
    out = {"shape": np.array(SHAPE), "tags": np.array(["init_W64_s2", "sharp_W64", "sharp_W256", "sharp_W512"])}
    nets = {"init_W64_s2": mg.make_net(64, 4, 2)[0]}
    for W in (64, 256, 512):
        net = mg.T_NeRF(W, 4)
        r = net.load_state_dict(sharp_state(W), strict=True)
        assert not r.missing_keys and not r.unexpected_keys
        nets[f"sharp_W{W}"] = net
    for tag, net in nets.items():
        s, hm = columns(net)
        out[f"{tag}_P_Surf_sum"], out[f"{tag}_Est_HM"] = np.asarray(s, dtype=np.float64), np.asarray(hm, dtype=np.float64)
        print(f"{tag}: mean P_Surf sum {s.mean():.4f}, Est_HM in [{hm.min():.4f}, {hm.max():.4f}]", flush=True)
    path = os.path.join(mg.OUT, "height_columns.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
