#!/usr/bin/env python
"""A/B timing of the captured training step's per-step inputs on an MI355X: the W = 256, S = 96 training step (MSE loss, free phase) captured as one hipGraph
launch with the batch drawn inside the graph (GraphedTrainStep(tool, loader=...)) from a synthetic ray table of 1e6 rows, at R = 512 (the reference's default
batch, main_lite.py:73) and R = 4096 rays:
  (a) host:    inputs="host" - both jitter vectors, the random sun rays and Adam's scalars drawn with numpy / torch on the host, packed, uploaded through the
               pinned ring and dealt out by a multi-tensor copy between two replays;
  (b) device:  inputs="device" - step_inputs.DeviceStepInputs draws them inside the graph (two more kernel nodes): a replay takes no host input.
One fresh process per leg, the legs alternated (a b a b ...), `--runs` of each per size; every process under its own time limit, and the driver stops at the
first one that fails or overruns (nothing more is started on the device).  A leg warms up (`--warmup` steps: engine build, capture, first replays), then times
`--steps` steps with a host clock between two device synchronisations; the host time per step is the same loop's clock before the closing synchronisation.
Reported per size and leg: the median of the runs' ms per step, their range, the median host ms per step.

    python tools/step_inputs_ab.py [--steps 200] [--warmup 6] [--runs 3] [--rows 1000000] [--leg-timeout 240] [--out profiles/r19/step_inputs_ab.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

W, NC, S = 256, 4, 96
SIZES = [512, 4096]
LEGS = ["host", "device"]


def leg(a):
    import season_nerf_amd as sn
    from loader_ab import H4, WC, synthetic_table
    dev = torch.device("cuda")
    table = synthetic_table(a.rows).to(dev)
    net = sn.T_NeRF(W, NC)
    net.load_state_dict(sn.synthetic_state_dict(net, 0, bn_stats="identity"))
    net = net.to(dev).train()
    args = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=True, Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=NC)
    ev = sn.All_in_One_Eval(args, dev, 10, False, None, H4, WC)
    tool = sn.Net_tool(net, ev, 10 ** -4.86, total_steps=a.steps + a.warmup + 8, writer=None)
    np.random.seed(0); torch.manual_seed(0)
    ld = sn.DeviceRayLoader(table, a.rays, seed=0, drop_last=True)
    step = sn.GraphedTrainStep(tool, loader=ld, warmup=2, inputs=a.leg, seed=0)
    for k in range(a.warmup):
        step(None, k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(a.steps):
        loss = step(None, a.warmup + k)
    t_host = time.perf_counter() - t0
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    assert step.graph is not None and not step.disabled and (step.inputs is not None) == (a.leg == "device")
    res = {"leg": a.leg, "rays": a.rays, "ms_per_step": round(ms, 3), "host_ms_per_step": round(t_host * 1e3 / a.steps, 3), "steps": a.steps,
           "colour_loss": float(loss["Color"][0])}
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out")
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--rays", type=int, default=4096)
    a = ap.parse_args()
    if a.warmup < 3:
        ap.error("--warmup must cover the two eager steps and the capture (>= 3)")
    if a.leg:
        return leg(a)
    lines = [f"# W = {W}, S = {S}, MSE loss, captured step with the batch drawn inside the graph; table of {a.rows} rows; {a.steps} timed steps after {a.warmup}; "
             f"{a.runs} runs per leg, alternated; ms per step"]
    ok = True
    for rays in SIZES:
        got = {w: [] for w in LEGS}
        for n in range(a.runs * len(LEGS)):
            which = LEGS[n % len(LEGS)]
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--rays", str(rays), "--steps", str(a.steps), "--warmup", str(a.warmup),
                   "--rows", str(a.rows)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
            except subprocess.TimeoutExpired:
                lines.append(f"R = {rays} {which}: failed: over its limit of {a.leg_timeout} s")
                ok = False
                break                                  # a leg that hangs ends the study: nothing more is started on the device
            out = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
            if r.returncode != 0 or not out:
                lines.append(f"R = {rays} {which}: failed: exit {r.returncode}: {r.stderr[-400:]!r}")
                ok = False
                break
            res = json.loads(out[-1])
            got[which].append(res)
            lines.append(f"R = {rays} {'a host' if which == 'host' else 'b device'} run {len(got[which])}: {res['ms_per_step']:.3f}   host {res['host_ms_per_step']:.3f}   "
                         f"(last colour loss {res['colour_loss']:.6f})")
            print(lines[-1], flush=True)
        if not ok:
            break
        med = {}
        for which in LEGS:
            ms = [x["ms_per_step"] for x in got[which]]
            med[which] = statistics.median(ms)
            lines.append(f"R = {rays} {'a host' if which == 'host' else 'b device'}: median {med[which]:.3f}  range {min(ms):.3f} .. {max(ms):.3f}  "
                         f"host median {statistics.median(x['host_ms_per_step'] for x in got[which]):.3f}")
        a_ms, b_ms = ([x["ms_per_step"] for x in got[w]] for w in LEGS)
        if max(b_ms) < min(a_ms):
            verdict = f"(b) is faster than (a) beyond the legs' own spread: {med['host'] - med['device']:.3f} ms per step between the medians"
        elif max(a_ms) < min(b_ms):
            verdict = f"(b) is SLOWER than (a) beyond the legs' own spread: {med['device'] - med['host']:.3f} ms per step between the medians"
        else:
            verdict = "(b) is not faster than (a) beyond the legs' own spread (the ranges overlap)"
        lines.append(f"R = {rays}: {verdict}")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
