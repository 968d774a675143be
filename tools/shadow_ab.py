#!/usr/bin/env python
"""A/B timing of the reference's shadow test on an MI355X, on its full walk: 42 x 42 sun directions x 64 x 64 ground points x 96 samples
(main_eval_region.py:77-84 with the lattice of Sample_Walk_Points_Shadow: 7.2e6 rays, 6.9e8 evaluations of trunk, density head and solar branch).
  (a) kernel:     `Test_Shadow_Points(full_return=False)`: one `season_nerf::shadow_walk` launch per chunk of rays, eight sums per ray;
  (b) per_sample: the same scores the way the package could form them before: `forward_Solar` on the materialised sample points of a chunk of rays,
                  `get_PV`, torch reductions on the device (no host array: the most favourable form of that path).
Each leg is a fresh process under its own time limit (a leg that overruns is killed and reported as such; the other legs still run).  A leg warms up on a
slice of the suns, then times `--reps` synchronised runs of the whole walk.  One JSON line per weight set (also written to --out).

    python tools/shadow_ab.py [--sets sharp_W256 sharp_W512] [--reps 3] [--suns 42] [--ground 64] [--leg-timeout 300] [--out FILE]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import season_nerf_amd as sn                                  # noqa: E402
from season_nerf_amd import shadow_eval as SE                 # noqa: E402
from surface_ab import H4, WC, state                          # noqa: E402

S = 96


def lattices(n_suns, n_ground):
    """all_walking_points and ground_points of Sample_Walk_Points_Shadow (mg_Shadow_Eval.py:62,67)."""
    az = np.linspace(0, 360, n_suns, endpoint=False)
    suns = np.array([(el, a) for el in np.linspace(5, 90, n_suns) for a in az])                # elevation-major, azimuth without its end point
    xy = np.linspace(-1, 1, n_ground)
    ground = np.array([(x, y) for x in xy for y in xy])
    return suns, ground


def kernel_scores(net, suns, ground, dev):
    none = suns[:0]
    return SE.Test_Shadow_Points(net, none, none, none, suns, ground, WC, H4, dev, Z_points=S, full_return=False)["Full"]


def per_sample_scores(net, suns, ground, dev, chunk=1 << 16):
    """The scores from per-sample arrays of a chunk of rays at a time: sample points, forward_Solar, get_PV, reductions in float64 on the device."""
    tops64, bots64, orig = SE._sun_rays(suns, ground, WC, H4)
    M, G = tops64.shape[:2]
    top, bot = SE._f32(tops64, dev).reshape(-1, 3), SE._f32(bots64, dev).reshape(-1, 3)
    sun = SE._f32(orig, dev).unsqueeze(1).expand(M, G, 3).reshape(-1, 3)
    tv = sn.evaluator.sample_parameters_on(dev, S, eval_mode=True)
    tot = torch.zeros(5, dtype=torch.float64, device=dev)
    off = torch.zeros((), dtype=torch.float64, device=dev)
    with torch.no_grad():
        for i in range(0, M * G, chunk):
            j = min(M * G, i + chunk)
            n = j - i
            p, delta = SE._ray_samples(top[i:j], bot[i:j], tv, S, True)
            rho, vis, _ = net.forward_Solar(p.reshape(-1, 3), sun[i:j].unsqueeze(1).expand(n, S, 3).reshape(-1, 3), torch.zeros(n * S, 4, device=dev))
            pv = sn.get_PV(rho.reshape(n, S, 1), delta.reshape(n, S, 1).contiguous()).reshape(n, S)
            vis = vis.reshape(n, S)
            ex, es = pv > .5, vis > .5
            d = pv.double() - vis.double()
            ne, nv = ex.sum(1), es.sum(1)
            tot += torch.stack([(ex & es).sum().double(), ne.sum().double(), nv.sum().double(), (d * d).sum(), d.abs().sum()])
            off += (ne - nv).abs().sum().double()
        tot, off = tot.cpu().numpy(), float(off)
    return SE._scores_from_sums(tot[0], tot[1], tot[2], tot[3], tot[4], float(M * G) * S, off / (M * G))


def leg(a):
    if not torch.cuda.is_available():
        sys.exit("shadow_ab: needs an MI355X (a time taken anywhere else says nothing)")
    dev = torch.device("cuda")
    W, sd = state(a.set)
    net = sn.T_NeRF(W, 4)
    net.load_state_dict(sd)
    net.precision = "bf16x3"
    net = net.to(dev).eval()
    suns, ground = lattices(a.suns, a.ground)
    f = kernel_scores if a.leg == "kernel" else per_sample_scores
    f(net, suns[:: max(1, len(suns) // 16)], ground, dev)      # warm-up: every kernel and shape of the loop
    torch.cuda.synchronize()
    ts, scores = [], None
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = f(net, suns, ground, dev)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    print("LEG " + json.dumps({"leg": a.leg, "weights": a.set, "width": W, "rays": int(len(suns) * len(ground)), "seconds": [round(t, 3) for t in ts],
                               "median_s": round(statistics.median(ts), 3), "scores": {k: float(v) for k, v in scores.items()}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["sharp_W256", "sharp_W512"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--suns", type=int, default=42)
    ap.add_argument("--ground", type=int, default=64)
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--leg", choices=["kernel", "per_sample"])
    ap.add_argument("--set")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    lines = []
    for name in a.sets:
        res = {}
        for which in ("kernel", "per_sample"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--set", name, "--reps", str(a.reps), "--suns", str(a.suns), "--ground", str(a.ground)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
            except subprocess.TimeoutExpired:
                res[which] = {"failed": f"over its limit of {a.leg_timeout} s"}
                break                          # a leg that hangs ends the study: nothing more is started on the device
            got = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not got:
                res[which] = {"failed": f"exit {r.returncode}", "stderr": r.stderr[-400:]}
                break
            res[which] = json.loads(got[-1])
        line = {"weights": name, "suns": a.suns ** 2, "ground_points": a.ground ** 2, "samples": S, "precision": "bf16x3", "reps": a.reps, **res}
        if all("median_s" in res.get(k, {}) for k in ("kernel", "per_sample")):
            line["ratio_of_medians"] = round(res["kernel"]["median_s"] / res["per_sample"]["median_s"], 4)
            line["max_abs_score_diff"] = max(abs(res["kernel"]["scores"][k] - res["per_sample"]["scores"][k]) for k in res["kernel"]["scores"])
        print(json.dumps(line), flush=True)
        lines.append(line)
        if any("failed" in v for v in res.values()):
            break
    if a.out and lines:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
