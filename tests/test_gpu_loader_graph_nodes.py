"""The captured training step that draws its batch inside the graph (trainer.GraphedTrainStep(tool, loader=...)) under the guard of
tests/test_gpu_graph_nodes.py: the graph holds KERNEL nodes only (a MEMCPY / MEMSET node makes replays compute garbage on ROCm 7.2), and the
loader's two kernels are among them - the draw is part of the graph, not a copy in front of it.  The runtime's own DOT print, in a child process: the
switch is read at HIP start-up."""
import glob
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import numpy as np, torch
import season_nerf_amd as sn
from oracle import season_nerf_oracle as orc
from test_gpu_loader import _ray_table, WC, H4
from test_net_tool import _args
rng = np.random.Generator(np.random.PCG64(3))
hm = rng.uniform(-0.8, 0.6, (24, 24))
train = sn.DeviceRayLoader(torch.from_numpy(_ray_table(rng, 500)).cuda(), 48, seed=1, drop_last=True)
val = sn.DeviceRayLoader(torch.from_numpy(_ray_table(rng, 200)).cuda(), 48, seed=2)
tool = sn.T_NeRF_Net_Tool(_args(20, n_saves=3, use_mse=True), hm, hm, "cuda", H4, WC, train_loader=train, val_loader=val, use_graph=True)
tool.network.load_state_dict(orc.init_weights(64, 4, 1))
n = 0
for s_ in range(20):
    tool.step()
    n += int(tool._graphed is not None and tool._graphed.graph is not None)
torch.cuda.synchronize()
print("replayed", n, "draws", train.get_state()[2], flush=True)
"""


@pytest.mark.gpu
def test_captured_steps_with_the_draw_inside_hold_kernel_nodes_only(tmp_path):
    """20 steps, two captures (the DSM-prior phase and the free phase): hundreds of kernel nodes each, the loader's draw and advance kernels among them, not
    one memory-operation node; every step - eager warm-up or replay - took one batch from the loader."""
    env = dict(os.environ, DEBUG_HIP_GRAPH_DOT_PRINT="1")
    env.pop("SNERF_TRAIN_MEMOPS", None)
    r = subprocess.run([sys.executable, "-c", CHILD % (REPO, REPO)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert re.findall(r"replayed (\d+) draws (\d+)", r.stdout) == [("16", "20")], r.stdout
    dots = sorted(glob.glob(os.path.join(str(tmp_path), "graph_*dot_print*")))
    assert len(dots) == 2, (dots, r.stderr[-500:])
    for d in dots:
        s = open(d).read()
        labels = re.findall(r'label="\d+\n([^\n"]*)', s)
        assert len(labels) > 100, (d, len(labels))
        memops = [l for l in labels if re.search(r"memcpy|memset", l, re.I)]
        assert not memops, f"{os.path.basename(d)}: {len(memops)} memory-operation nodes among {len(labels)}: {sorted(set(memops))}"
        assert sum("loader_draw_kernel" in l for l in labels) == 1 and sum("loader_advance_kernel" in l for l in labels) == 1, sorted(set(labels))[:40]
