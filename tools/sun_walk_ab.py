#!/usr/bin/env python
"""A/B timing of the sun walk on an MI355X: M sun directions x T seasons of one view,
  (a) `render_sun_season_walk`: one field pass with the solar branch run M times, one grid-compositing launch;
  (b) what the package offered before: M times `_render_by_dir_device` (a complete field pass) followed by the sweep kernel.
bf16x3, init-law weights; the two are run alternately and the medians of the synchronised wall times reported; the images of (a) and (b) are compared
once.  One JSON line per width (also written to --out).

    python tools/sun_walk_ab.py [--widths 256 512] [--size 256 256 96] [--suns 12] [--times 12] [--reps 7] [--out FILE]
    python tools/sun_walk_ab.py --once a|b ...      one un-timed pass of one side: the workload for a profiler run (rocprofv3 ... -- python tools/sun_walk_ab.py --once a)
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import season_nerf_amd as sn                                  # noqa: E402
from season_nerf_amd import render as R_                      # noqa: E402
from oracle import season_nerf_oracle as orc                  # noqa: E402

WC = np.array([41.29, -95.9, 300.0])
H4 = np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])
VIEW = (70, 20)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--widths", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--size", type=int, nargs=3, default=[256, 256, 96])
    ap.add_argument("--suns", type=int, default=12)
    ap.add_argument("--times", type=int, default=12)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--once", choices=["a", "b"])
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sun_walk_ab: needs an MI355X (a time taken anywhere else says nothing)")
    dev = torch.device("cuda")
    size = tuple(a.size)
    suns = [(25.0 + 5.0 * j, (30.0 * j) % 360.0) for j in range(a.suns)]
    times = [k / a.times for k in range(a.times)]
    lines = []
    for W in a.widths:
        net = sn.T_NeRF(W, 4)
        net.load_state_dict(orc.init_weights(W, 4, 2))
        net.precision = "bf16x3"
        net = net.to(dev).eval()

        def side_a():
            return sn.render_sun_season_walk(net, VIEW, suns, times, size, WC, H4, dev)[0]

        def side_b():
            with torch.no_grad():
                tim = torch.tensor(np.stack([sn.encode_time(t) for t in times]), dtype=torch.float32, device=dev)
                cls = net.get_class_only(tim).cpu().numpy()
                out = []
                for s in suns:
                    d = R_._render_by_dir_device(net, VIEW, s, times[0], size, WC, H4, dev, False)
                    out.append(R_._sweep(d, cls, "Est_Solar_Vis")["shaded"])
                return torch.stack(out).reshape(len(suns), len(times), size[0], size[1], 3)

        if a.once:
            (side_a if a.once == "a" else side_b)()      # warm-up: code objects, the walk stream
            torch.cuda.synchronize()
            (side_a if a.once == "a" else side_b)()
            torch.cuda.synchronize()
            continue
        ia, ib = side_a(), side_b()                      # warm-up of every shape, and the comparison of the results
        torch.cuda.synchronize()
        diff = float((ia - ib).abs().max())
        del ia, ib
        ta, tb = [], []
        for _ in range(a.reps):
            for f, ts in ((side_a, ta), (side_b, tb)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
        ma, mb = statistics.median(ta), statistics.median(tb)
        line = {"width": W, "size": list(size), "suns": a.suns, "times": a.times, "precision": "bf16x3", "walk_ms_median": round(ma, 3), "loop_ms_median": round(mb, 3),
                "ratio": round(ma / mb, 4), "walk_ms": [round(t, 2) for t in ta], "loop_ms": [round(t, 2) for t in tb], "max_abs_image_diff": diff}
        print(json.dumps(line), flush=True)
        lines.append(line)
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
