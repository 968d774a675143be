"""Time snerf_group_forward with the split per-ray kernel (mode 0, csrc/kernels_group.hip) and the one-wave kernel (mode 1, csrc/kernels.hip):
HIP events around 200 back-to-back launches on one stream, per width and number of groups.  n_groups = 1 and 32 are the renderers' single-time,
single-sun case; 4096 is the benchmark's.   python tools/group_kernel_ab.py [--launches 200] [--groups 1 32 4096]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import season_nerf_amd as sn                      # noqa: E402
from oracle import season_nerf_oracle as orc      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--groups", type=int, nargs="+", default=[1, 32, 4096])
    ap.add_argument("--widths", type=int, nargs="+", default=[256, 64])
    a = ap.parse_args()
    L = sn._lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for W in a.widths:
        net = sn.T_NeRF(W, 4)
        net.load_state_dict(orc.init_weights(W, 4, 0))
        model = net.to("cuda").eval().device_model()
        for n in a.groups:
            rng = np.random.Generator(np.random.PCG64(n))
            tim = torch.tensor(rng.uniform(-1, 1, (n, 4)), dtype=torch.float32, device="cuda")
            sun = rng.uniform(0, 1, (n, 3))
            sun = torch.tensor(sun / np.linalg.norm(sun, axis=1, keepdims=True), dtype=torch.float32, device="cuda")
            cls, raw, sky = (torch.empty(n, k, device="cuda") for k in (4, 3, 3))
            call = lambda: sn._lib.check(L.snerf_group_forward(model, n, tim.data_ptr(), sun.data_ptr(), cls.data_ptr(), raw.data_ptr(), sky.data_ptr(), st), "group")
            res = {}
            for rep in range(3):                                  # modes alternated, three times each; the best of the three is reported
                for mode in (1, 0):
                    sn._lib.check(L.snerf_set_group_kernel(mode), "mode")
                    for _ in range(20):
                        call()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.launches):
                        call()
                    e1.record()
                    torch.cuda.synchronize()
                    res.setdefault(mode, []).append(e0.elapsed_time(e1) * 1e3 / a.launches)
            fmt = lambda v: " ".join(f"{x:.2f}" for x in v)
            print(f"W={W} n_groups={n}: one wave {min(res[1]):.2f} us per launch ({fmt(res[1])}), split {min(res[0]):.2f} us ({fmt(res[0])})", flush=True)
    sn._lib.check(L.snerf_set_group_kernel(0), "mode")


if __name__ == "__main__":
    main()
