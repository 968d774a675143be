#!/usr/bin/env python
"""A/B timing of the reference's solar audit on an MI355X: one view at the reference's own size (128, 128, 64) under the 24 sun directions of `advanced_solar`
(6 azimuths x 4 elevations, mg_Advanced_Solar.py:47-48), i.e. 2.5e7 secondary rays of 64 samples; sharp W = 256 weights, bf16x3.
  (a) renders:  24 x `component_render_by_dir(include_exact_solar=True)` and the reference's own scoring on the host arrays (`eval_solar_data` on a plain dict):
                what a user of the package had to do before;
  (b) pieces:   the sun walk (one field pass for the 24 suns), `_exact_solar_visibility` per sun (tops and bottoms through torch, `ray_visibility`), PS from
                one compositing launch and torch scoring on the device: the best the pieces allowed without the audit kernel;
  (c) audit:    `audit_by_dir`: the sun walk, one compositing launch, one `season_nerf::solar_audit` launch per sun.
Each leg is a fresh process under its own time limit; the legs are alternated (a, b, c, a, b, c, ...) so that a drift of the machine meets all of them.  A leg
warms up on two suns, then times `--reps` synchronised runs of all 24.  Reported: per leg the median and the spread (min, max) of all its timed runs, and
whether the counts agree.  One JSON line (also written to --out).

    python tools/solar_audit_ab.py [--rounds 3] [--reps 2] [--size 128 128 64] [--set sharp_W256] [--leg-timeout 300] [--out FILE]
"""
import argparse
import importlib
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
from season_nerf_amd import render as R_                      # noqa: E402
from surface_ab import H4, WC, state                          # noqa: E402

SA = importlib.import_module("season_nerf_amd.solar_audit")   # the module (the package exports its function `solar_audit` under the same name)
VIEW = (70.0, 90.0)
SUNS = [(float(el), float(az)) for az in np.linspace(0, 360, 6, endpoint=False) for el in np.linspace(15, 90, 4, endpoint=False)]
LEGS = ("renders", "pieces", "audit")


def leg_renders(net, suns, size, dev):
    out = []
    for s in suns:
        d = sn.component_render_by_dir(net, VIEW, s, 0.0, size, WC, H4, dev, include_exact_solar=True, skip_weightless=None)
        out.append(SA.eval_solar_data({k: d[k] for k in ("Exact_Solar", "Est_Solar_Vis", "Rho", "Deltas")}))      # float64 host arrays, as the reference holds them
    return out


def leg_pieces(net, suns, size, dev):
    S = size[2]
    with torch.no_grad():
        d = R_._sun_walk_device(net, VIEW, suns, 0.0, size, WC, H4, dev)
        R = d["Rho"].shape[0]
        ps = SA._composite_ps(R, S, d["top"], d["bot"], d["tv"], d["Rho"], d["Est_Solar_Vis"], net._stream())
        pts = d["World_Points"].reshape(-1, 3)
        out = []
        for j, s in enumerate(suns):
            sunv = R_.world_angle_2_local_vec(s[0], s[1], WC, H4)
            ex = R_._exact_solar_visibility(net, pts, R_._f32(sunv, dev), S, zero_oob=True, sun64=sunv).reshape(R, S)
            es = d["Solar_Vis_All"][j].reshape(R, S)
            out.append(SA._confusion(ex > .5, es > .5, (ex * ps).sum(1) > .3, (es * ps).sum(1) > .3, lambda m: int(m.sum().item())))
    return out


def leg_audit(net, suns, size, dev):
    a = sn.audit_by_dir(net, VIEW, suns, size, WC, H4, dev)
    return [a.confusion(j) for j in range(len(suns))]


def leg(a):
    if not torch.cuda.is_available():
        sys.exit("solar_audit_ab: needs an MI355X (a time taken anywhere else says nothing)")
    dev = torch.device("cuda")
    W, sd = state(a.set)
    net = sn.T_NeRF(W, 4)
    net.load_state_dict(sd)
    net.precision = "bf16x3"
    net = net.to(dev).eval()
    f = {"renders": leg_renders, "pieces": leg_pieces, "audit": leg_audit}[a.leg]
    size = tuple(a.size)
    f(net, SUNS[:2], size, dev)      # warm-up: every kernel and shape of the loop
    torch.cuda.synchronize()
    ts, conf = [], None
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        conf = f(net, SUNS, size, dev)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    flat = [[c[fam][k] for fam in ("All_Solar_Vis", "Surface_Solar_Vis") for k in ("TP", "TN", "FP", "FN")] for c in conf]
    print("LEG " + json.dumps({"leg": a.leg, "seconds": [round(t, 4) for t in ts], "counts": flat}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="sharp_W256")
    ap.add_argument("--size", nargs=3, type=int, default=[128, 128, 64])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--leg", choices=LEGS)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    times, counts, failed = {k: [] for k in LEGS}, {}, None
    for _ in range(a.rounds):
        for which in LEGS:
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--set", a.set, "--reps", str(a.reps), "--size"] + [str(x) for x in a.size]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
            except subprocess.TimeoutExpired:
                failed = {which: f"over its limit of {a.leg_timeout} s"}
                break                          # a leg that hangs ends the study: nothing more is started on the device
            got = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not got:
                failed = {which: f"exit {r.returncode}", "stderr": r.stderr[-400:]}
                break
            res = json.loads(got[-1])
            times[which] += res["seconds"]
            counts[which] = np.array(res["counts"])
        if failed:
            break
    line = {"weights": a.set, "view": VIEW, "size": a.size, "suns": len(SUNS), "precision": "bf16x3", "rounds": a.rounds, "reps_per_process": a.reps}
    for k in LEGS:
        if times[k]:
            line[k] = {"median_s": round(statistics.median(times[k]), 4), "min_s": round(min(times[k]), 4), "max_s": round(max(times[k]), 4), "runs": len(times[k])}
    if failed:
        line["failed"] = failed
    if all(k in counts for k in LEGS):
        line["max_count_difference_to_renders"] = {k: int(np.abs(counts[k] - counts["renders"]).max()) for k in ("pieces", "audit")}
        line["samples_per_sun"] = int(a.size[0] * a.size[1] * a.size[2])
    print(json.dumps(line), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
