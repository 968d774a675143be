"""A/B of the fused loss terms for Barron's adaptive colour loss (season_nerf::loss_terms_all, `fused_loss="all"`) against the tensor-op
formulation (`fused_loss="default"`) on the training step:  python tools/loss_terms_ab.py [--out FILE]

Legs, one process each (a leg that fails or hangs ends the study): {default, all} x {eager, captured} x {free phase, DSM-prior phase} x
R in {512, 4096}, W = 256, S = 96, adaptive loss (the reference's own run: Use_MSE_loss off, jump_start on; its default batch is 512 rays).
Per leg:
  step ms   wall time per step over --steps steps after --warmup, one synchronisation at the end;
  host ms   time the Python thread spends inside the step call (no synchronisation): what the step costs the host;
  nodes     captured legs: kernel nodes of the step's hipGraph as the runtime prints it (DEBUG_HIP_GRAPH_DOT_PRINT) = kernel launches per step
            (the eager step of the same configuration launches the same kernels, plus its per-step uploads).
"""
import argparse
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

W, NC, S = 256, 4, 96
WC, H4 = np.array([41.29, -95.9, 300.0]), np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])
LEGS = [(R, phase, how, mode) for R in (512, 4096) for phase in ("free", "prior") for how in ("eager", "captured") for mode in ("default", "all")]


def leg(a):
    import season_nerf_amd as sn
    from season_nerf_amd.adaptive_loss import AdaptiveLossFunction
    dev = torch.device("cuda")
    R, prior = a.rays, a.phase == "prior"
    hm = np.random.Generator(np.random.PCG64(3)).uniform(-0.8, 0.6, (128, 128))
    net = sn.T_NeRF(W, NC, HM=hm) if prior else sn.T_NeRF(W, NC)
    net.load_state_dict(sn.synthetic_state_dict(net, 0, bn_stats="identity"))
    net = net.to(dev).train()
    args = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=False, Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=NC)
    mk = lambda dims, s0, slo: AdaptiveLossFunction(dims, torch.float32, dev, alpha_hi=2.99, alpha_init=2.0, scale_init=s0, scale_lo=slo)      # Net_Tool_2.py:69-82
    ada = [mk(3, .03, .01), mk(1, .5, .05)] if prior else mk(3, .03, .01)
    n_total = a.steps + a.warmup + 8
    ev = sn.All_in_One_Eval(args, dev, 4 * n_total, prior, ada, H4, WC)
    ev.fused_loss = a.mode
    tool = sn.Net_tool(net, ev, 10 ** -4.86, total_steps=n_total, lr_alpha_scale=30.0, writer=None)
    rng = np.random.Generator(np.random.PCG64(5))
    t = lambda x: torch.tensor(x, dtype=torch.float32, device=dev)
    sun = rng.uniform(0.1, 1, (R, 3)); sun /= np.linalg.norm(sun, axis=1, keepdims=True)
    tau = rng.uniform(0, 1, (R, 2))
    batch = {"Top": t(np.concatenate([rng.uniform(-1, 1, (R, 2)), np.ones((R, 1))], 1)), "Bot": t(np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1)),
             "Sun_Angle": t(sun), "Time_Encoded": t(np.stack([np.cos(6.28 * tau[:, 0]), np.sin(6.28 * tau[:, 0]), np.cos(6.28 * tau[:, 1]), np.sin(6.28 * tau[:, 1])], 1)),
             "GT_Color": t(rng.uniform(0, 1, (R, 3)))}
    np.random.seed(0); torch.manual_seed(0)
    if a.how == "captured":
        step = sn.GraphedTrainStep(tool, batch, warmup=2)
        run = lambda k: step(batch, k)
    else:
        run = lambda k: tool.train_step(batch, k)
    for k in range(a.warmup):
        run(k)
    torch.cuda.synchronize()
    host = 0.0
    t0 = time.perf_counter()
    for k in range(a.steps):
        h0 = time.perf_counter()
        loss = run(a.warmup + k)
        host += time.perf_counter() - h0
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    if a.how == "captured":
        assert step.graph is not None and not step.disabled
    nodes = None
    dots = glob.glob("graph_*dot_print*")
    if dots:
        nodes = len(re.findall(r'label="\d+\n', open(sorted(dots)[-1]).read()))
    res = {"rays": R, "phase": a.phase, "how": a.how, "mode": a.mode, "ms_per_step": round(ms, 3), "host_ms_per_step": round(host * 1e3 / a.steps, 3), "nodes": nodes,
           "fused": getattr(loss, "wvec", None) is not None, "color_ada": float(loss["Color_ada"][0])}
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out")
    ap.add_argument("--rays", type=int)
    ap.add_argument("--phase", choices=["free", "prior"])
    ap.add_argument("--how", choices=["eager", "captured"])
    ap.add_argument("--mode", choices=["default", "all"])
    a = ap.parse_args()
    if a.warmup < 3:
        ap.error("--warmup must cover the two eager steps and the capture (>= 3)")
    if a.rays:
        return leg(a)
    lines = [f"# W = {W}, S = {S}, adaptive colour loss; {a.steps} timed steps after {a.warmup}; rays phase how mode: step ms | host ms | graph nodes (= kernel launches per step) | last Color_ada"]
    for R, phase, how, mode in LEGS:
        cmd = [sys.executable, os.path.abspath(__file__), "--rays", str(R), "--phase", phase, "--how", how, "--mode", mode, "--steps", str(a.steps), "--warmup", str(a.warmup)]
        env = dict(os.environ)
        env.pop("SNERF_FUSED_LOSS", None)
        if how == "captured":
            env["DEBUG_HIP_GRAPH_DOT_PRINT"] = "1"
        with tempfile.TemporaryDirectory() as d:
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout, cwd=d, env=env)
            except subprocess.TimeoutExpired:
                lines.append(f"{R} {phase} {how} {mode}: failed: over its limit of {a.leg_timeout} s")
                break                                  # a leg that hangs ends the study: nothing more is started on the device
        got = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
        if r.returncode != 0 or not got:
            lines.append(f"{R} {phase} {how} {mode}: failed: exit {r.returncode}: {r.stderr[-400:]!r}")
            break
        res = json.loads(got[-1])
        assert res["fused"] == (mode == "all"), res
        lines.append(f"{R:5d} {phase:5s} {how:8s} {mode:7s}: {res['ms_per_step']:8.3f} | {res['host_ms_per_step']:7.3f} | {res['nodes'] if res['nodes'] is not None else '-':>4} | {res['color_ada']:.5f}")
        print(lines[-1], flush=True)
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
