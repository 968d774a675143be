#!/usr/bin/env python
"""A/B timing of the training loop's data path on an MI355X: the W = 256, 4096 rays x 96 samples training step (MSE loss, free phase) captured as one
hipGraph launch, fed in four ways from a synthetic ray table of 1e6 rows:
  (a) host:     the reference's way (mg_run_NeRF.py:74-84,229-264): a torch DataLoader(shuffle=True, num_workers=4) over the host copy of the table, one
                __getitem__ per row; a second one over a dataset that draws t.rand(4) per sun-check ray (the arithmetic of NN_loaders/mg_SC_loader.py:17-21);
                data_to_dict, upload, DSM_Distance.get_Dist; the batch is then copied into the captured step's buffers;
  (b) device:   DeviceRayLoader.next() (with the DSM distances) feeding the same captured step;
  (c) in_graph: GraphedTrainStep(tool, loader=...): the draw is the graph's first two kernels, nothing travels per step;
  (d) resident: the captured step fed ONE batch that already sits on the device: the floor.  Run three times: the run-to-run spread.
Each leg is a fresh process under its own time limit (a leg that overruns is killed and reported as such, and nothing more is started).  A leg warms up
(`--warmup` steps: engine build, capture, first replays), then times `--steps` steps with a host clock between two device synchronisations.  One line per
leg: milliseconds per step.

    python tools/loader_ab.py [--steps 40] [--warmup 6] [--rows 1000000] [--leg-timeout 300] [--out profiles/r15/loader_ab.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

W, NC, R, S = 256, 4, 4096, 96
WC, H4 = np.array([41.29, -95.9, 300.0]), np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])
LEGS = ["host", "device", "in_graph", "resident", "resident", "resident"]


def synthetic_table(n, seed=0):
    """[n, 22] float32 on the host: rays through the cube from z = +1 to z = -1, 40 images' worth of sun directions and times."""
    g = torch.Generator().manual_seed(seed)
    u = lambda *sh: torch.rand(*sh, generator=g)
    img = torch.randint(0, 40, (n,), generator=g)
    sun = torch.nn.functional.normalize(u(40, 3) * 0.9 + 0.1, dim=1)[img]
    tau = u(40, 2)[img] * 6.28
    time_enc = torch.stack([torch.cos(tau[:, 0]), torch.sin(tau[:, 0]), torch.cos(tau[:, 1]), torch.sin(tau[:, 1])], 1)
    return torch.cat([torch.randint(0, 512, (n, 2), generator=g).float(), u(n, 2) * 2 - 1, torch.ones(n, 1), u(n, 2) * 2 - 1, -torch.ones(n, 1),
                      torch.nn.functional.normalize(u(n, 3) - 0.5, dim=1), sun, time_enc, torch.ones(n, 1), u(n, 3)], 1).contiguous()


class RowDataset(torch.utils.data.Dataset):
    """One table row per item, as the reference's colour loader hands them out."""

    def __init__(self, rows):
        self.rows = rows

    def __len__(self):
        return self.rows.shape[0]

    def __getitem__(self, i):
        return self.rows[i]


class SunCheckDataset(torch.utils.data.Dataset):
    """A random ray through the cube per item: four uniforms, top at z = +1, bottom at z = -1."""

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        r = torch.rand(4)
        return torch.tensor([r[0] * 2.0 - 1.0, r[1] * 2.0 - 1.0, 1.0]), torch.tensor([r[2] * 2.0 - 1.0, r[3] * 2.0 - 1.0, -1.0])


class Cycle:
    """next() over a DataLoader, restarted at StopIteration (Net_tool.get_data)."""

    def __init__(self, dl):
        self.dl, self.it = dl, iter(dl)

    def next(self):
        try:
            return next(self.it)
        except StopIteration:
            self.it = iter(self.dl)
            return next(self.it)


def leg(a):
    import season_nerf_amd as sn
    dev = torch.device("cuda")
    host_rows = synthetic_table(a.rows)
    if a.leg == "host":                            # the worker processes start here, before this process opens the GPU (they never touch it)
        mk = lambda ds: torch.utils.data.DataLoader(ds, batch_size=R, shuffle=True, num_workers=4)
        colour, sc = Cycle(mk(RowDataset(host_rows))), Cycle(mk(SunCheckDataset(a.rows)))
    net = sn.T_NeRF(W, NC)
    net.load_state_dict(sn.synthetic_state_dict(net, 0, bn_stats="identity"))
    net = net.to(dev).train()
    args = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=True, Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=NC)
    ev = sn.All_in_One_Eval(args, dev, 10, False, None, H4, WC)
    tool = sn.Net_tool(net, ev, 10 ** -4.86, total_steps=a.steps + a.warmup + 8, writer=None)
    hm = np.random.Generator(np.random.PCG64(3)).uniform(-0.8, 0.6, (128, 128))
    dist = sn.DSM_Distance(hm, hm * 0.9, S, dev)
    np.random.seed(0); torch.manual_seed(0)
    if a.leg == "host":
        def get():
            d = sn.raytable.data_to_dict(colour.next())
            d["SC_Top"], d["SC_Bot"] = sc.next()
            d = {k: v.to(dev) for k, v in d.items()}
            d["Dist_to_Surf_GT"], d["Dist_to_Surf_Prior"] = dist.get_Dist(d["Top"], d["Bot"])
            return d
        step = sn.GraphedTrainStep(tool, get(), warmup=2)
        run = lambda k: step(get(), k)
    else:
        table = host_rows.to(dev)
        if a.leg == "device":
            ld = sn.DeviceRayLoader(table, R, seed=0, drop_last=True, dsm_distance=dist)
            step = sn.GraphedTrainStep(tool, ld.next(), warmup=2)
            run = lambda k: step(ld.next(), k)
        elif a.leg == "in_graph":
            ld = sn.DeviceRayLoader(table, R, seed=0, drop_last=True)
            step = sn.GraphedTrainStep(tool, loader=ld, warmup=2)
            run = lambda k: step(None, k)
        else:
            batch = {k: v.contiguous() for k, v in sn.raytable.data_to_dict(table[:R]).items()}
            step = sn.GraphedTrainStep(tool, batch, warmup=2)
            run = lambda k: step(batch, k)
    for k in range(a.warmup):
        run(k)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(a.steps):
        loss = run(a.warmup + k)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    assert step.graph is not None and not step.disabled
    res = {"leg": a.leg, "ms_per_step": round(ms, 3), "steps": a.steps, "rows": a.rows, "colour_loss": float(loss["Color"][0])}
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--rows", type=int, default=1000000)
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--out")
    ap.add_argument("--leg", choices=sorted(set(LEGS)))
    a = ap.parse_args()
    if a.warmup < 3:
        ap.error("--warmup must cover the two eager steps and the capture (>= 3)")
    if a.leg:
        return leg(a)
    lines = [f"# W = {W}, {R} rays x {S} samples, MSE loss, captured step; table of {a.rows} rows; {a.steps} timed steps after {a.warmup}; ms per step"]
    floor = []
    for n, which in enumerate(LEGS):
        cmd = [sys.executable, os.path.abspath(__file__), "--leg", which, "--steps", str(a.steps), "--warmup", str(a.warmup), "--rows", str(a.rows)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.leg_timeout)
        except subprocess.TimeoutExpired:
            lines.append(f"{which}: failed: over its limit of {a.leg_timeout} s")
            break                                  # a leg that hangs ends the study: nothing more is started on the device
        got = [ln[4:] for ln in r.stdout.splitlines() if ln.startswith("LEG ")]
        if r.returncode != 0 or not got:
            lines.append(f"{which}: failed: exit {r.returncode}: {r.stderr[-400:]!r}")
            break
        res = json.loads(got[-1])
        name = {"host": "a host", "device": "b device", "in_graph": "c in_graph", "resident": f"d resident run {len(floor) + 1}"}[which]
        if which == "resident":
            floor.append(res["ms_per_step"])
        lines.append(f"{name}: {res['ms_per_step']:.3f}   (last colour loss {res['colour_loss']:.6f})")
        print(lines[-1], flush=True)
    if len(floor) == 3:
        lines.append(f"d spread: min {min(floor):.3f} max {max(floor):.3f} (max - min {max(floor) - min(floor):.3f})")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
