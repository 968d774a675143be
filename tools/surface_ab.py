#!/usr/bin/env python
"""A/B timing of the height map on an MI355X: `Quick_Run_Net.get_DSM(size)`
  (a) density_only=True: one `season_nerf::ray_surface` launch (density-only network, compositing inside the kernel, early-out behind opaque surfaces);
  (b) density_only=False, what the package offered before: the whole field program, its per-sample arrays, `composite_kernel` and a torch sum.
The two are run alternately in one process and the medians and spreads of the synchronised wall times reported; the two height maps are compared once.
Weight sets: the sharp W = 256 and W = 512 fixtures (opaque surfaces: the early-out has something to skip) and init-law weights forced to bf16x3 (fog: it
has nothing).  The early-out's share of rays is the share whose `carry` with the early-out is below its `carry` without (flags bit 2): rays with a pass skipped.
One JSON line per weight set (also written to --out).

    python tools/surface_ab.py [--size 512 512] [--pairs 20] [--sets sharp_W256 sharp_W512 init_W256] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import season_nerf_amd as sn                                  # noqa: E402
from season_nerf_amd import render as R_                      # noqa: E402
from oracle import season_nerf_oracle as orc                  # noqa: E402

WC = np.array([41.29, -95.9, 300.0])
H4 = np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])
GOLDEN = os.path.join(REPO, "tests", "golden")
HEAD = ("G_NeRF_net.fc10Sigma.weight", "G_NeRF_net.fc10Sigma.bias")


def state(name):
    kind, W = name.split("_W")
    if kind == "init":
        return int(W), orc.init_weights(int(W), 4, 2)
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))
    t = dict(np.load(os.path.join(GOLDEN, str(g["source"])), allow_pickle=False))
    return int(W), {k[3:]: torch.tensor(v) * (float(g["g"]) if k[3:] in HEAD else 1.0) for k, v in t.items() if k.startswith("sd_")}


def spread(ts):
    q = statistics.quantiles(ts, n=4)
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3), "iqr": round(q[2] - q[0], 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--pairs", type=int, default=20)
    ap.add_argument("--sets", nargs="+", default=["sharp_W256", "sharp_W512", "init_W256"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("surface_ab: needs an MI355X (a time taken anywhere else says nothing)")
    dev = torch.device("cuda")
    size = tuple(a.size)
    args = SimpleNamespace(n_samples=96, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=True, Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=4)
    lines = []
    for name in a.sets:
        W, sd = state(name)
        net = sn.T_NeRF(W, 4)
        net.load_state_dict(sd)
        net.precision = "bf16x3"
        net = net.to(dev).eval()
        qr = sn.Quick_Run_Net(net, args, WC, H4, dev, use_full_solar=False)
        new, old = qr.get_DSM(size, density_only=True), qr.get_DSM(size)      # warm-up of every shape, and the comparison of the results
        torch.cuda.synchronize()
        m = np.isfinite(old)
        diff = float(np.abs(new[m] - old[m]).max()) if (np.isfinite(new) == m).all() else float("nan")
        with torch.no_grad():
            d = qr._get_input_dict([90, 0], [90, 0], 0.0, size, None)
            c_early = R_.ray_surface(net, d["Top"], d["Bot"], 96).carry
            c_full = R_.ray_surface(net, d["Top"], d["Bot"], 96, early_out=False).carry
            share = float((c_early < c_full).float().mean())
            opaque = float((c_full > 18).float().mean())
        ta, tb = [], []
        for _ in range(a.pairs):
            for f, ts in ((lambda: qr.get_DSM(size, density_only=True), ta), (lambda: qr.get_DSM(size), tb)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
        line = {"weights": name, "width": W, "size": list(size), "samples": 96, "rays": int(d["Top"].shape[0]), "precision": "bf16x3", "pairs": a.pairs,
                "density_only_ms": spread(ta), "full_ms": spread(tb), "ratio_of_medians": round(statistics.median(ta) / statistics.median(tb), 4),
                "rays_with_a_pass_skipped": round(share, 4), "rays_past_depth_18": round(opaque, 4), "max_abs_height_diff": diff}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
