#!/usr/bin/env python
"""A/B timing of one film frame of the reference (T_NeRF_Eval_Utils/mg_movie_maker.py capture_frame_advanced) on an MI355X: 256 x 256 rays x 96 samples,
three seasons, pitch 12 and yaw 35 degrees about the cube's centre.
  (a) walk:       `frame_walk`: one `season_nerf::frame_walk` launch for the three seasons, sixteen floats per ray;
  (b) per_sample: the route there was before: per season `T_NeRF.forward` on the materialised sample points of a chunk of rays, the density zeroed outside
                  the cube, PE / PV / PS and the shaded sum in float64 on the device (no host array: the most favourable form of that path).
Each leg is a fresh process under its own time limit (a leg that overruns is killed and reported as such, and nothing more is started).  A leg warms up on a
sixteenth of the rays, then times `--reps` synchronised renders of the frame.  The walk leg also reports the early-out's share of skipped passes, counted
from the depth every ray has walked after 32 and after 64 samples (two launches on the truncated sample vectors, early-out off) and the kernel's own vote:
the rays of a workgroup (4, or 2 at width 512) skip the passes behind the first pass end at which all of them stand beyond optical depth 18.  One JSON line
per weight set (also written to --out).

    python tools/frame_ab.py [--sets sharp_W256 sharp_W512] [--reps 20] [--size 256] [--leg-timeout 240] [--out FILE]
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
from season_nerf_amd import movie as MV                       # noqa: E402
from surface_ab import state                                  # noqa: E402

S = 96
SUN = np.array([0.3, -0.2, 0.93]) / np.sqrt(np.sum(np.array([0.3, -0.2, 0.93]) ** 2))
TIMES = (0.1, 0.45, 0.8)
FRAME = (np.array([0.0, 0.0, 0.0]), (0.9, 0.9, 1.1), 12.0, 35.0)


def planes(size, dev):
    top, bot, delta = MV.frame_end_planes(FRAME[0], FRAME[1], FRAME[2], FRAME[3], (size, size, S))
    f = lambda a: torch.tensor(a, device=dev).reshape(-1, 3).contiguous()
    return f(top), f(bot), float(delta)


def walk_frame(net, top, bot, delta, dev):
    fw = MV.frame_walk(net, top, bot, S, delta, SUN, times=TIMES)
    return fw.rgb, fw.height_map((top.shape[0], 1)).reshape(-1)


def per_sample_frame(net, top, bot, delta, dev, chunk=1 << 16):
    """eval_rays_advanced the way the package could form it before: the whole network once per season on the sample points of a chunk of rays."""
    R = top.shape[0]
    tv = sn.evaluator.sample_parameters_on(dev, S, eval_mode=True, include_end_pt=True)
    sun = torch.tensor(SUN, dtype=torch.float32, device=dev).reshape(1, 3)
    rgb = torch.empty(len(TIMES), R, 3, dtype=torch.float64, device=dev)
    hm = torch.empty(R, dtype=torch.float64, device=dev)
    lin = torch.linspace(0, 2, S, dtype=torch.float64, device=dev).reshape(1, S)
    with torch.no_grad():
        for k, tf in enumerate(TIMES):
            tim = torch.tensor(sn.encode_time(tf), dtype=torch.float32, device=dev).reshape(1, 4)
            for i in range(0, R, chunk):
                j = min(R, i + chunk)
                n = j - i
                t = tv.reshape(1, S, 1)
                p = top[i:j].unsqueeze(1) * (1.0 - t) + bot[i:j].unsqueeze(1) * t
                rho, col, vis, sky, _, _ = net(p.reshape(-1, 3), sun.expand(n * S, 3), tim.expand(n * S, 4))
                y = torch.where((p.abs() > 1).any(2), torch.zeros(1, dtype=torch.float64, device=dev), rho.reshape(n, S).double()) * delta
                c = torch.cumsum(torch.cat([torch.zeros_like(y[:, :1]), y], 1), 1)
                ps = torch.exp(-c[:, :-1]) * (1.0 - torch.exp(-y))
                vis = vis.reshape(n, S, 1).double()
                rgb[k, i:j] = (ps.unsqueeze(2) * (vis + (1.0 - vis) * sky[0].double().reshape(1, 1, 3)) * col.reshape(n, S, 3).double()).sum(1)
                if k == len(TIMES) - 1:
                    hm[i:j] = (ps * lin).sum(1)
    return rgb, hm


def skipped_share(net, top, bot, delta, dev):
    """Passes the early-out skips / passes of the frame, from the depth walked after 32 and after 64 samples and the workgroup's vote."""
    from season_nerf_amd.network import _ops
    tv = sn.evaluator.sample_parameters_on(dev, S, eval_mode=True, include_end_pt=True)
    sun = torch.tensor(SUN, dtype=torch.float32, device=dev)
    tim = torch.tensor(sn.encode_time(TIMES[0]), dtype=torch.float32, device=dev).reshape(1, 4)
    cls, _, sky = net._groups(tim, sun.reshape(1, 3))
    per = 2 if net.layer_width == 512 else 4
    R = top.shape[0]
    pad = (-R) % per
    depth = []
    for n in (32, 64):
        d = _ops().frame_walk(net.device_model(), top, bot, tv[:n].contiguous(), delta, sun, sky[0].contiguous(), cls.contiguous(), 6)[:, 14]
        depth.append(torch.cat([d, torch.full((pad,), 1e30, device=dev)]).reshape(-1, per).min(1).values > 18.0)
    groups = depth[0].numel()
    skipped = 2 * int(depth[0].sum()) + int((depth[1] & ~depth[0]).sum())
    return skipped / (3.0 * groups)


def leg(a):
    if not torch.cuda.is_available():
        sys.exit("frame_ab: needs an MI355X (a time taken anywhere else says nothing)")
    dev = torch.device("cuda")
    W, sd = state(a.set)
    net = sn.T_NeRF(W, 4)
    net.load_state_dict(sd)
    net.precision = "bf16x3"
    net = net.to(dev).eval()
    top, bot, delta = planes(a.size, dev)
    f = walk_frame if a.leg == "walk" else per_sample_frame
    f(net, top[::16].contiguous(), bot[::16].contiguous(), delta, dev)      # warm-up: every kernel of the loop
    torch.cuda.synchronize()
    ts, out = [], None
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f(net, top, bot, delta, dev)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    res = {"leg": a.leg, "weights": a.set, "width": W, "rays": int(top.shape[0]), "ms": [round(t * 1e3, 2) for t in ts], "median_ms": round(statistics.median(ts) * 1e3, 2),
           "min_ms": round(min(ts) * 1e3, 2), "opaque_rays": None}
    if a.leg == "walk":
        res["skipped_passes_share"] = round(skipped_share(net, top, bot, delta, dev), 4)
        res["opaque_rays"] = round(float((MV.frame_walk(net, top, bot, S, delta, SUN, times=TIMES).opacity > 0.99).double().mean()), 4)
    if a.dump:
        torch.save({"rgb": out[0].cpu(), "hm": out[1].cpu()}, a.dump)
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["sharp_W256", "sharp_W512"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out")
    ap.add_argument("--leg", choices=["walk", "per_sample"])
    ap.add_argument("--set")
    ap.add_argument("--dump")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    import tempfile
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        for name in a.sets:
            res = {}
            for which in ("walk", "per_sample"):
                dump = os.path.join(tmp, f"{name}_{which}.pt")
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--set", name, "--reps", str(a.reps), "--size", str(a.size), "--dump", dump]
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
            line = {"weights": name, "frame": [a.size, a.size, S], "seasons": len(TIMES), "precision": "bf16x3", "reps": a.reps, **res}
            if all("median_ms" in res.get(k, {}) for k in ("walk", "per_sample")):
                line["ratio_of_medians"] = round(res["walk"]["median_ms"] / res["per_sample"]["median_ms"], 4)
                x, y = torch.load(os.path.join(tmp, f"{name}_walk.pt")), torch.load(os.path.join(tmp, f"{name}_per_sample.pt"))
                line["max_abs_image_diff"] = float((x["rgb"] - y["rgb"]).abs().max())
                line["max_abs_hm_diff"] = float((x["hm"] - y["hm"]).abs().max())
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
