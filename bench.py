#!/usr/bin/env python3
"""Headline benchmark: BASELINE.json configs[1] - forward render of 4096 rays x 96 samples through
T_NeRF(256, 4) (eval-mode BN, random weights of the reference's init law), synthetic rays.

A "step" = one pass of the hot path over one ray batch: per-ray group network (season classes + sky colour)
-> fused field network (sampling + PE + SIREN MLP + heads) -> wave-scan compositing, inputs resident in HBM.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--full] [--dump-outputs DIR]

A plain run sets up, pre-warms, warms up, times K steps and prints the headline line.  `--full` adds every other
measurement (see below and `--help`); `--dump-outputs DIR` writes the outputs of the last timed step as DIR/<name>.npy (float32;
inputs and weights are seeded, so two builds can be compared output for output).

N > 1: one process per GPU.  Either the driver starts the ranks (`python -m torch.distributed.run --nproc-per-node N ... bench.py
--gpus N`: RANK / WORLD_SIZE set), or a bare `python bench.py --gpus N` starts them itself - as a CHILD process running
torch.distributed.run, before this process has touched the GPU - and exits with the child's status.

Prints ONE JSON line on rank 0.  At N = 1 with `--full` the line also carries the training step of BASELINE configs[2] as extra keys
(`train_ms_per_step`, `train_roofline`, `train_cpu_baseline`; MSE colour loss = the reference-pinned path), the evaluator-seam
time (`eval_seam_ms`) and the 512 x 512 x 96 + 12-step sweep render, all measured outside the headline timed region.  Multi-GPU: every rank renders its own 4096-ray tile (weak scaling, rays are
independent) and the rendered RGB tiles are all-gathered over RCCL, 8 steps per asynchronous collective (the tile
exchange of a tiled novel-view render); value = total ray-samples of all ranks / max-over-ranks time.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

# The GPU path needs ONE host thread.  On the test boxes the process sees 256 hardware threads but a 16-CPU cgroup quota:
# OpenMP / BLAS worker pools woken by a tiny host op (the reference's host-side sun-ray generator runs every training step)
# spin, burn the quota, and the launching thread gets throttled for multiples of the 10 ms scheduler tick - measured as
# 24 ms -> 40-50 ms per training step.  Pools are therefore kept at one thread unless the user says otherwise; the CPU
# baseline below raises torch's thread count explicitly, to the cgroup quota.
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ.setdefault(_v, "1")

import numpy as np   # noqa: E402
import torch         # noqa: E402


def host_info():
    """What the CPU baseline ran on: model name, hardware threads visible, cgroup quota, affinity - the hosts of the GPU boxes differ
    (the same oracle code measured 5.7e4 ... 3.3e5 ray-samples/s across rounds), so the baseline names its host."""
    model = "unknown"
    try:
        for line in open("/proc/cpuinfo"):
            if line.lower().startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except Exception:
        pass
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        quota = None if q == "max" else int(q) / int(per)
    except Exception:
        pass
    return {"cpu_model": model, "hardware_threads": os.cpu_count(), "affinity": len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else None,
            "cgroup_cpu_quota": quota}


def host_cpus():
    """CPUs this process may actually use: cgroup v2 quota, then affinity, then the machine count."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return n

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def _local_device():
    """The GPU of this rank: LOCAL_RANK.  SNERF_BENCH_DEVICE overrides it - the two-rank rehearsal on a ONE-GPU box puts every rank on device 0
    (tests/test_gpu_two_ranks.py), together with SNERF_BENCH_BACKEND=gloo (RCCL refuses two ranks on one device; gloo reduces device tensors)."""
    return int(os.environ.get("SNERF_BENCH_DEVICE", os.environ.get("LOCAL_RANK", "0")))


def _init_group(dist, dev):
    backend = os.environ.get("SNERF_BENCH_BACKEND", "nccl")          # "nccl" IS RCCL on ROCm
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group(backend)

R, S, W, NC = 4096, 96, 256, 4
# algorithmic forward cost per ray-sample at W=256, C=4, S=96 (2 FLOP per MAC, per-ray branches amortised)
FLOP_PER_SAMPLE = 2 * (743936 + 71040 / 96.0)
PEAK_BF16_DENSE = 2.5e15   # MI355X_MICROARCH.md: dense bf16 MFMA peak
PEAK_INT8_DENSE = 5.0e15   # int8 MFMA: the cycles of the bf16 form at twice the K (MI355X_MICROARCH.md, Matrix cores)


DTYPES = {"i8x3": "i8x3 (16-bit fixed point as two int8 digits on v_mfma_i32_32x32x32_i8, exact int32 accumulate, fp32 epilogue)",
          "bf16x3": "bf16x3 (3-term split bf16 MFMA, fp32 accumulate)", "bf16": "bf16 (one bf16 MFMA per product, fp32 accumulate; fast mode)"}
KERNELS = {"i8x3": "snerf::mlp_i8x2_kernel<256,0> (fused field network, int8 digits, two waves per SIMD)", "bf16x3": "snerf::mlp_kernel<0,256,0,false> (fused field network)",
           "bf16": "snerf::mlp_kernel<0,256,0,true> (fused field network, fast mode)"}
# executed matrix work per 32-point wave tile, in units of 65536 ops (= one 32x32x32 int8 MFMA = two 32x32x16 bf16 MFMAs)
MFMAS_PER_WAVE_TILE = {"i8x3": 2220, "bf16x3": 2220, "bf16": 772}
EXEC_NOTE = {"i8x3": "The kernel executes 3 int8 MFMAs (32x32x32) per 32-feature k-step (digit products T a, T b, L a): executed_tops are int8 "
                     "tera-ops/s against the 5,000 of the dense int8 peak.",
             "bf16x3": "The kernel executes 3 bf16 MFMAs per algorithmic product (error-compensated split) plus padding: executed_tops are bf16 TFLOP/s.",
             "bf16": "One bf16 MFMA per product (3 in the first layer): executed_tops are bf16 TFLOP/s."}


def synth(seed, dev):
    rng = np.random.Generator(np.random.PCG64(seed))
    top = np.concatenate([rng.uniform(-1, 1, (R, 2)), np.ones((R, 1))], 1)
    bot = np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1)
    sun = rng.uniform(0, 1, (R, 3))
    sun /= np.linalg.norm(sun, axis=1, keepdims=True)
    tau, d = rng.uniform(0, 1, R), rng.uniform(0, 1, R)
    tim = np.stack([np.cos(2 * np.pi * tau), np.sin(2 * np.pi * tau), np.cos(2 * np.pi * d), np.sin(2 * np.pi * d)], 1)
    t = lambda a: torch.tensor(a, dtype=torch.float32, device=dev)
    return {"Top": t(top), "Bot": t(bot), "Sun_Angle": t(sun), "Time_Encoded": t(tim)}


def cpu_baseline():
    """The CPU oracle (a torch-CPU restatement of the reference path, oracle/season_nerf_oracle.py) timed on the host
    cores of this box on a bounded sample of the same workload."""
    from oracle import season_nerf_oracle as orc
    torch.set_num_threads(min(host_cpus(), 32))   # more threads only slow these small GEMMs down
    sd = orc.init_weights(W, NC, 0)
    data = {k: v.cpu() for k, v in synth(0, "cpu").items()}
    sub = lambda n: {k: v[:n] for k, v in data.items()}
    with torch.no_grad():
        orc.eval_rays(sd, sub(128), S, False)              # warm-up
        n, ts = R, []                                      # the whole 4096-ray batch per repetition
        t0 = time.perf_counter()
        orc.eval_rays(sd, sub(n), S, False)
        ts.append(time.perf_counter() - t0)
        reps = int(min(max(3, np.ceil(12.0 / ts[0])), 12))  # >= 12 s of CPU work in all (hosts differ 6x), at most 12 repetitions
        for _ in range(reps - 1):
            t0 = time.perf_counter()
            orc.eval_rays(sd, sub(n), S, False)
            ts.append(time.perf_counter() - t0)
    t = float(np.median(ts))
    return {"value": n * S / t, "unit": "ray-samples/s", "cores": torch.get_num_threads(), "kind": "port",
            "sample": f"{n} rays x {S} samples of the same workload (eval-mode forward render, fp32 torch-CPU oracle), "
                      f"median of {reps} after warm-up", "seconds_per_repetition": ts, "torch_threads": torch.get_num_threads(),
            "torch_interop_threads": torch.get_num_interop_threads(), **host_info()}


TRAIN_KERNEL = "snerf::gemm_rows16_kernel<8,4,1,0>"


FLOP_PER_SAMPLE_512 = 2 * (2896896 + 273152 / 96.0)        # SURVEY 8d at W = 512
W512_KERNELS = {"i8x3": "snerf::mlp_i8_kernel<0,512,0> (fused field network at W = 512, int8 digits, one wave per SIMD, activations in AGPRs)",
                "bf16x3": "snerf::mlp_ks_kernel<512,0> (fused field network at W = 512, bf16x3, every layer's K split over a wave pair)"}


def w512_kernel_roofline(dev, d, tv, launches=20, precision="auto"):
    """The fused field kernel of the reference's default width (main_lite.py:80) on the benchmark's rays, T_NeRF(512, 4) with init-law weights:
    `snerf::mlp_i8_kernel<0,512,0>` (precision auto / i8x3) or `snerf::mlp_ks_kernel<512,0>` (bf16x3: what a converged checkpoint runs on).
    Returns (summary, roofline object); HIP events on the stream the C ABI launches on (torch's current stream)."""
    import season_nerf_amd as sn
    L = sn._lib.lib()
    n5 = sn.T_NeRF(512, NC)
    n5.load_state_dict(sn.synthetic_state_dict(n5, 0))
    n5.precision = precision
    n5 = n5.to(dev).eval()                          # "auto": the fused int8-digit kernel for these weights
    m5 = n5.device_model()
    e = lambda *s_: torch.empty(*s_, device=dev)
    cls, rho, sv, col = torch.softmax(torch.rand(R, NC, device=dev), 1), e(R * S), e(R * S), e(R * S, 3)
    fo = sn._lib.FieldOut(d_rho=rho.data_ptr(), d_solar_vis=sv.data_ptr(), d_col=col.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    run5 = lambda: sn._lib.check(L.snerf_field_forward_rays(m5, 0, R, S, d["Top"].data_ptr(), d["Bot"].data_ptr(), tv.data_ptr(), 1, d["Sun_Angle"].data_ptr(),
                                                           cls.data_ptr(), C.byref(fo), st), "field")
    for _ in range(2):
        run5()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        run5()
    e1.record()
    torch.cuda.synchronize()
    ms5 = e0.elapsed_time(e1) / launches
    flop5 = FLOP_PER_SAMPLE_512 * R * S
    pr5 = n5.resolved_precision
    tr5 = None
    try:
        tr5 = json.load(open(_profile_file("w512_traffic.json" if pr5 == "i8x3" else "w512_bf16x3_traffic.json")))["bytes_per_launch"]
    except Exception:
        pass
    i8 = pr5 == "i8x3"
    peak = PEAK_INT8_DENSE if i8 else PEAK_BF16_DENSE        # the pipe the kernel issues on
    roof = {"bound": "mfma", "kernel": W512_KERNELS[pr5], "achieved": flop5 / (ms5 * 1e-3) / 1e12, "peak": peak / 1e12, "unit": "TFLOP/s",
            "frac": flop5 / (ms5 * 1e-3) / peak, "frac_of_bf16_peak": flop5 / (ms5 * 1e-3) / PEAK_BF16_DENSE,
            "traffic": tr5, "kernel_ms": ms5, "algorithmic_flop": flop5}
    summ = {"field_kernel_ms": ms5, "precision": f"{precision} -> {pr5}", "ray_samples_per_s_kernel": R * S / (ms5 * 1e-3)}
    return summ, roof


def sharp_state_dict(width):
    """Weights WITH SURFACES: tests/golden/trained_W{width}.npz (the reference's own training loop) with the density head scaled by the g of
    tests/golden/sharp_W{width}.npz (mean max-PS per ray >= 0.5 by the reference's eval; tools/make_sharp_golden.py).  Arrays only."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden")
    g = np.load(os.path.join(here, f"sharp_W{width}.npz"), allow_pickle=False)
    t = np.load(os.path.join(here, f"trained_W{width}.npz"), allow_pickle=False)
    head = ("G_NeRF_net.fc10Sigma.weight", "G_NeRF_net.fc10Sigma.bias")
    sd = {k[3:]: torch.tensor(t[k]) * (float(g["g"]) if k[3:] in head else 1.0) for k in t.files if k.startswith("sd_")}
    return sd, float(g["g"]), float(g["max_ps"].mean())


def converged_row(dev, d, tv, width, launches=20):
    """The benchmark's batch (4096 rays x 96 samples) rendered with weights that have SURFACES in them, class default precision: what `auto`
    resolves to for a converged checkpoint, and what a step (per-ray networks + field network + compositing) costs then."""
    import season_nerf_amd as sn
    sd, gain, mps = sharp_state_dict(width)
    net = sn.T_NeRF(width, NC)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    prec = net.resolved_precision
    from types import SimpleNamespace
    eargs = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=True, Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=NC)
    ev = sn.All_in_One_Eval(eargs, dev, 10, False, None, np.eye(4), np.zeros(3))
    with torch.no_grad():
        for _ in range(2):
            r = ev.render_summary(d, net) if hasattr(ev, "render_summary") and prec is not None else ev.eval(d, net, 0, False)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            r = ev.render_summary(d, net) if hasattr(ev, "render_summary") and prec is not None else ev.eval(d, net, 0, False)
        e1.record()
        torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / launches
    flop = (FLOP_PER_SAMPLE if width == 256 else FLOP_PER_SAMPLE_512) * R * S
    est = net.i8_estimate()
    row = {"weights": f"sharp_W{width}: trained_W{width}.npz (the reference's training loop), density head x{gain:g}; mean max-PS per ray {mps:.2f}",
           "precision_resolved": prec if prec is not None else "layer-wise engine", "i8_rgb_pred": est["rgb_pred"], "ms_per_step": ms, "value": R * S / (ms * 1e-3),
           "unit": "ray-samples/s",
           "roofline": {"bound": "mfma", "achieved": flop / (ms * 1e-3) / 1e12, "peak": PEAK_BF16_DENSE / 1e12, "unit": "TFLOP/s", "frac": flop / (ms * 1e-3) / PEAK_BF16_DENSE,
                        "note": "whole step by HIP events (per-ray networks + field network + compositing), algorithmic FLOPs of SURVEY 8d"}}
    if width == 512:      # what these weights cost before round 6: the layer-wise engine (reached today through the one-term mode, which has no fused kernel at 512)
        net.precision = "bf16"
        assert not net.fused
        with torch.no_grad():
            ev.eval(d, net, 0, False)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(5):
                ev.eval(d, net, 0, False)
            e1.record()
            torch.cuda.synchronize()
        row["layerwise_engine_ms_per_step"] = e0.elapsed_time(e1) / 5
    return row


SIGMA_FLOP_PER_SAMPLE = 2 * 524800.0          # trunk fc1..fc9 + density head, W = 256 (16 128 + 6 x 65 536 + 81 664 + 32 768 + 128 ... = 524 800 MACs)
SIGMA_FLOP_PER_SAMPLE_512 = 2 * 2030848.0     # the same at W = 512: 63 x 512 + 6 x 512^2 + 575 x 512 + 512 x 256 + 256


def renderer_a_row(dev, net):
    """Renderer A (Quick_Run_Net.render_img, exact solar on - its default in the reference, Quick_Run.py:62) for one 256 x 256 x 96 image, end to end (ray grid,
    primary render, secondary rays, the three images back on the host): as it ships - samples without compositing weight get no secondary ray - and with a
    secondary ray for every sample (`skip_weightless=None`, the reference's loop)."""
    import time
    from types import SimpleNamespace
    import season_nerf_amd as sn
    WC, H4 = np.array([41.29, -95.9, 300.0]), np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])
    eargs = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=True, Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=NC)
    row = {"image": "256x256x96, view (70, 20), sun (40, 110)", "precision_resolved": net.resolved_precision}
    for key, skip in (("ms", 1e-9), ("ms_every_sample", None)):
        qr = sn.Quick_Run_Net(net, eargs, WC, H4, dev, use_full_solar=True, skip_weightless=skip)
        qr.render_img((70, 20), (40, 110), 0.3, 48)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        qr.render_img((70, 20), (40, 110), 0.3, 256)
        torch.cuda.synchronize()
        row[key] = (time.perf_counter() - t0) * 1e3
        if skip is not None:
            walked, of = qr.eval_tool.last_exact_solar_rays
            row["secondary_rays_walked"], row["secondary_rays"] = walked, of
    return row


def exact_solar_bench(dev, net, sizes=((256, 256, 96), (512, 512, 96)), layerwise_too=False):
    """The exact-solar pass (Eval_Tools_2.py:255-295 / mg_Img_Eval.py:57-70; the DEFAULT of both reference renderers): for every sample of every
    primary ray a secondary ray towards the sun, S density-only evaluations each - R S^2 in all - as `season_nerf::ray_visibility` launches
    (one float out per secondary ray).  Timed by HIP events on the launch stream, primary render excluded."""
    import season_nerf_amd as sn
    from season_nerf_amd import render as R_
    WC, H4 = np.array([41.29, -95.9, 300.0]), np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])
    out = {}
    for size in sizes:
        Hh, Ww, Ss = size
        with torch.no_grad():
            dd = R_._render_by_dir_device(net, (80, 0), (30, 90), 0.25, size, WC, H4, dev, False)
            pts = dd["World_Points"].reshape(-1, 3)
            sunv = R_.world_angle_2_local_vec(30, 90, WC, H4)
            sun_d = torch.tensor(sunv, dtype=torch.float32, device=dev)
            vis = R_._exact_solar_visibility(net, pts[: 1 << 16], sun_d, Ss, zero_oob=True, sun64=sunv)          # warm-up
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            vis = R_._exact_solar_visibility(net, pts, sun_d, Ss, zero_oob=True, sun64=sunv)
            e1.record()
            torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        n = pts.shape[0] * Ss
        fl = (SIGMA_FLOP_PER_SAMPLE if net.layer_width == 256 else SIGMA_FLOP_PER_SAMPLE_512) * n
        i8 = net.resolved_precision == "i8x3"
        peak = PEAK_INT8_DENSE if i8 else PEAK_BF16_DENSE          # the pipe the kernel issues on
        row = {"ms": ms, "secondary_rays": int(pts.shape[0]), "sigma_samples": int(n), "sigma_samples_per_s": n / (ms * 1e-3), "mean_visibility": float(vis.mean()),
               "roofline": {"bound": "mfma", "achieved": fl / (ms * 1e-3) / 1e12, "peak": peak / 1e12, "unit": "TFLOP/s",
                            "frac": fl / (ms * 1e-3) / peak, "frac_of_bf16_peak": fl / (ms * 1e-3) / PEAK_BF16_DENSE}}
        if layerwise_too:      # the composition this kernel replaced at W = 512 (render.py _visibility_layerwise: layer-wise density over 65 536-ray chunks + a transmittance scan)
            keep = net.precision
            net.precision = "bf16"                                  # the one-term mode has no fused kernel at 512: the layer-wise engine
            assert not net.fused
            sub = pts.shape[0] // 16                                # 1/16 of the secondary rays (a 64 x 64 x 96 image's worth): the composition is chunked by memory
            with torch.no_grad():
                R_._exact_solar_visibility(net, pts[:4096], sun_d, Ss, zero_oob=True, sun64=sunv)
                torch.cuda.synchronize()
                e0.record()
                vl = R_._exact_solar_visibility(net, pts[:sub], sun_d, Ss, zero_oob=True, sun64=sunv)
                e1.record()
                torch.cuda.synchronize()
            row["layerwise_composition_ms_extrapolated"] = e0.elapsed_time(e1) * 16
            row["layerwise_note"] = "measured on 1/16 of the secondary rays, x16; round 5's fixed 65 536-ray chunks asked for 435 GB here (out of memory): chunks are sized to ~12 GB now"
            row["layerwise_vs_kernel_max_abs_dev"] = float((vl - vis[:sub]).abs().max())
            net.precision = keep
            net.device_model()
            del vl
        out[f"{Hh}x{Ww}x{Ss}"] = row
        del dd, pts, vis
        torch.cuda.empty_cache()
    out["precision_resolved"] = net.resolved_precision
    out["note"] = (f"secondary-ray pass of include_exact_solar=True only (ray_visibility kernel); algorithmic MACs per secondary sample (trunk + density head): "
                   f"{int((SIGMA_FLOP_PER_SAMPLE if net.layer_width == 256 else SIGMA_FLOP_PER_SAMPLE_512) / 2)} at W = {net.layer_width}")
    return out


def sweep_kernel_roofline(dev, rays=512 * 512, T=12, launches=5):
    """`snerf::sweep_kernel` (csrc/kernels.hip; mg_Img_Eval.get_imgs_from_Img_Dict_t_step, :192-228) alone at configs[4]'s size: 512 x 512 rays x 96
    samples, 12 time steps per pass.  Algorithmic bytes: the 17 floats per sample it reads once for all T (rho, col_raw 3, adjust C x 3, solar_vis)
    + the [T, R, 3] x 2 + [R, 7] it writes.  HIP events on torch's current stream = the stream the op launches on."""
    import season_nerf_amd as sn
    sn.ops.load()
    g = torch.Generator(device=dev).manual_seed(1)
    rn = lambda *sh: torch.rand(*sh, device=dev, generator=g)
    top = torch.cat([rn(rays, 2) * 2 - 1, torch.ones(rays, 1, device=dev)], 1)
    bot = torch.cat([rn(rays, 2) * 2 - 1, -torch.ones(rays, 1, device=dev)], 1)
    tv = sn.sample_parameters(S, eval_mode=True).to(dev)
    rho, colr, adj, sv = rn(rays, S, 1) * 3, rn(rays, S, 3) - 0.5, rn(rays, S, NC, 3) - 0.5, rn(rays, S, 1)
    sky, cv = rn(3), torch.softmax(rn(T, NC), 1)
    run = lambda: torch.ops.season_nerf.composite_sweep(top, bot, tv, rho, colr, adj, sv, sky, cv, 0, False)
    run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        run()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / launches
    nbytes = 4.0 * (rays * S * (5 + 3 * NC) + 2 * T * rays * 3 + rays * 7)
    traffic = None
    try:
        traffic = json.load(open(_profile_file("sweep_traffic.json")))["bytes_per_launch"]
    except Exception:
        pass
    return {"bound": "hbm", "kernel": "snerf::sweep_kernel (512 x 512 rays x 96 samples, 12 time steps per pass)", "achieved": nbytes / (ms * 1e-3) / 1e9, "peak": 8000.0,
            "unit": "GB/s", "frac": nbytes / (ms * 1e-3) / 8e12, "traffic": traffic, "kernel_ms": ms, "algorithmic_bytes": nbytes}


def train_dominant_kernel(dev, launches=20, width=256):
    """The training step's dominant kernel on its own, live: the forward row GEMM of a 256 -> 256 SineLayer at M = 393 216 points
    (activation on load from the stored pre-activation of the layer below, BatchNorm column sums in the epilogue) - 21 of the
    step's launches, ~23 % of its time.  Algorithmic bytes: read Z_in, write Z_out = 4 M (K + N).  HIP events on the stream the
    C ABI launches on (torch's current stream)."""
    import season_nerf_amd as sn
    L = sn._lib.lib()
    M, K, N = R * S, width, width
    A = torch.randn(M, K, device=dev) * 4
    Wt = torch.randn(N, K, device=dev) / 16
    b = torch.randn(N, device=dev)
    out = torch.empty(M, N, device=dev)
    tab = torch.rand(2 * K, device=dev)
    stats = torch.zeros(2 * N, dtype=torch.float64, device=dev)
    sc = torch.empty(L.snerf_linear_scratch_bytes(N, K), dtype=torch.uint8, device=dev)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    run = lambda: sn._lib.check(L.snerf_linear_forward(M, K, N, A.data_ptr(), K, Wt.data_ptr(), b.data_ptr(), 30.0, out.data_ptr(), N, stats.data_ptr(), 1,
                                                      sc.data_ptr(), sc.numel(), tab.data_ptr(), K, st), "linear_forward")
    for _ in range(3):
        run()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        run()
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / launches * 1e3 - 5.0          # each call also runs the 5 us weight-split kernel (own launch, in the trace)
    nbytes = 4.0 * M * (K + N)
    traffic = None
    try:
        traffic = json.load(open(_profile_file("train_kernel_traffic.json")))["bytes_per_launch"]
    except Exception:
        pass
    if width != 256:
        traffic = None                                        # the committed counter passes are of the 256-wide kernel
    name = TRAIN_KERNEL if width == 256 else f"snerf::gemm_rows*_kernel (the row GEMM snerf_linear_forward selects for {width} -> {width})"
    return {"bound": "hbm", "kernel": name + f" (forward {width}->{width} SineLayer, activation on load + BatchNorm sums in the epilogue, M = 393216)",
            "achieved": nbytes / (us * 1e-6) / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": nbytes / (us * 1e-6) / 8e12, "traffic": traffic,
            "kernel_us": us, "algorithmic_bytes": nbytes, "launches_per_step": 21}


def bench_train(a, standalone=True):
    """BASELINE configs[2]: training step = zero_grad, get_loss (image rays + R random sun rays, train-mode BatchNorm, MSE
    colour loss by default - the path whose losses and gradients are pinned to the reference at this very size,
    tests/golden/train_W256_R4096_S96.npz; `--loss barron` selects the parity-unpinned adaptive loss), backward, gradient
    all-reduce over RCCL when N > 1, fused Adam.  Returns the result dict on rank 0 (None elsewhere).
    standalone=False: called from the render benchmark at N = 1 (no process group, its own step counts)."""
    from types import SimpleNamespace
    import season_nerf_amd as sn
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", _local_device())
    torch.cuda.set_device(dev)
    dist = None
    use_dist = standalone and (world > 1 or "RANK" in os.environ)      # under torch.distributed.run the RCCL path runs even with one rank
    if use_dist:
        import torch.distributed as dist
        _init_group(dist, dev)
    steps, warm = (min(a.steps, 20), min(a.warmup, 3)) if standalone else (12, 3)
    Wt = getattr(a, "width", W)
    net = sn.T_NeRF(Wt, NC)
    net.load_state_dict(sn.synthetic_state_dict(net, 0, bn_stats="identity"))        # reference init law, fresh BatchNorm
    net = net.to(dev).train()
    barron = a.loss == "barron"
    args = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=not barron, Use_Solar=True, sc_lambda=0.03,
                           number_low_frequency_cases=NC)
    WC, H4 = np.array([41.29, -95.9, 300.0]), np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])
    # Net_Tool_2.py:69: the colour loss object of the un-guided phase
    ada = sn.AdaptiveLossFunction(3, torch.float32, dev, alpha_hi=2.99, alpha_init=2.0, scale_init=0.03, scale_lo=0.01) if barron else None
    ev = sn.All_in_One_Eval(args, dev, 10, False, ada, H4, WC)
    d = synth(rank, dev)
    d["GT_Color"] = torch.rand(R, 3, device=dev)
    # the reference's optimisation step as the training seam runs it (trainer.Net_tool.train_step = mg_run_NeRF.py:288-326):
    # FusedAdam (all-reduces the flat gradient arena under data parallelism) + a second Adam on the loss object's parameters
    # (their gradients travel as one small all-reduce) + OneCycleLR on both
    tool = sn.Net_tool(net, ev, 10 ** -4.86, total_steps=steps + warm + 8, lr_alpha_scale=1000.0, writer=None)
    np.random.seed(rank)
    torch.manual_seed(rank)

    # --train-graph: one hipGraph launch per step; its first two calls are eager (they build the engine), the third captures - all before the timed region
    graphed = sn.GraphedTrainStep(tool, d, warmup=2) if getattr(a, "train_graph", False) else None

    def step():
        return graphed(d, 0) if graphed is not None else tool.train_step(d, 0)      # the loss dict; its total is formed once, after the timed region

    def total_of(loss):
        return sum(v.detach() * w for v, w in loss.values())

    step()                                   # builds the engine
    if a.bn_sync == "global" and use_dist:
        net._train_engine.sync_batchnorm(True)
    for _ in range(max(warm - 1, 0)):
        step()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    t0 = time.perf_counter()
    for i in range(steps):
        marks[i].record()
        tot = step()
    marks[steps].record()
    host_loop_ms = (time.perf_counter() - t0) / steps * 1e3  # wall time of the enqueue loop per step: includes back-pressure (the pinned upload ring
                                                             # lets the host run at most ~5 steps ahead, then it waits for the GPU) - NOT the host's own cost
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if use_dist:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    dt /= steps
    # what the HOST needs to enqueue one step (Python, dispatcher, C ABI, ~100 launches): every step issued onto an IDLE GPU
    # (synchronize first), so nothing the host waits for is in it; outside the timed region
    hq = []
    for _ in range(6):
        torch.cuda.synchronize()
        th = time.perf_counter()
        step()
        hq.append((time.perf_counter() - th) * 1e3)
    torch.cuda.synchronize()
    host_ms = sorted(hq)[len(hq) // 2]
    per_step = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(steps))     # stream time of each step (diagnostic)
    gemm = os.environ.get("SNERF_TRAIN_GEMM", "bf16x3")
    # algorithmic FLOPs: image rays 3 x forward; sun rays: trunk+heads+solar forward + 3 x solar/sky heads
    flop = R * S * (3 * FLOP_PER_SAMPLE + 2 * (524800 + 3 * 54656)) if Wt == 256 else None      # SURVEY 8d counts W = 256 only
    # HBM bytes the layer-wise design moves per step (every per-point layer is a pass over [points x width] fp32
    # arrays; per-ray branches are negligible).  Forward of a layer: one GEMM (read the pre-activation of the layer below -
    # the activation is applied on load - write Z); backward: activation backward (see bwd_bytes), then wgrad (read dZ, in)
    # and dgrad (read dZ, write d_in); heads: no activation passes.
    rows = {n: (o, i, "sine" if sine else "lin", bn) for n, o, i, sine, bn in sn.per_point_layer_shapes(net)}
    g_ = "G_NeRF_net."
    trunk = [g_ + f"fc{i}" for i in range(1, 10)]
    heads = [g_ + "fc10Col", g_ + "fc10Sigma"]
    solar = [g_ + "fc_solar_1", g_ + "fc_solar_2", g_ + "fc_solar_3", g_ + "fc_solar_4"]
    adjust = ["adjust_layer_1", "adjust_layer_2", "adjust_layer_3", "adjust_col"]

    aol = os.environ.get("SNERF_TRAIN_AOL", "1") != "0" and gemm != "fp32"

    def fwd_bytes(names):
        return sum((i + o) + (2 * o if (k == "sine" and not aol) else 0) for o, i, k, _ in (rows[n] for n in names))

    def bwd_bytes(names, dgrad_first=True):
        # activation backward of a SineLayer: fused into the epilogue of the (last) dgrad that produces its output gradient
        # (reads Z once: o), else a reduction sweep;
        # BatchNorm layers add the dZ computation (a sweep: read Z, dY, write dZ = 3 o - or folded into wgrad, see below)
        tot = 0
        for j, n in enumerate(names):
            o, i, k, bn = rows[n]
            if k == "sine":
                fused = aol
                tot += o if fused else (2 * o if bn else 3 * o)
                if bn:      # dZ: inside the weight-gradient kernel (reads Z, rewrites dY in place: 2 o) where the layer has <= 256 inputs
                    tot += 2 * o if (fused and i <= 256) else 3 * o
            tot += (o + i) + ((o + i) if (dgrad_first or j > 0) else 0)
        return tot
    img = fwd_bytes(trunk + heads + solar + adjust) + bwd_bytes(trunk, False) + bwd_bytes(heads) + bwd_bytes(adjust)
    sol = fwd_bytes(trunk + heads + solar) + bwd_bytes(solar, False)
    hbm_bytes = 4.0 * R * S * (img + sol)
    lname = "Barron adaptive loss" if barron else "MSE loss"
    traffic = None      # HBM bytes per step from the committed PMC passes of this same command (tools/profile_round.py)
    try:
        traffic = json.load(open(_profile_file("train_traffic.json")))["bytes_per_step"]
    except Exception:
        pass
    if rank == 0:
        out = {"metric": f"training image-ray-samples/s (4096 rays x 96 samples + 4096 sun rays per GPU, {lname}, fused Adam)",
               "value": world * R * S / dt, "unit": "ray-samples/s", "n_gpus": world, "steps": steps, "warmup": warm, "ms_per_step": dt * 1e3,
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
               "dtype": "f32 storage; " + ("bf16x3 split MFMA GEMMs (forward with activation on load, dgrad, wgrad)" if gemm != "fp32" else "fp32 MFMA GEMMs"),
               "data": "synthetic",
               "train_graph": graphed is not None,
               "config": {"workload": f"BASELINE configs[2]: training step 4096x96, T_NeRF({Wt},4) train-mode BatchNorm, solar branch on, {lname}"
                                      + ("" if Wt == 256 else " - at the reference's default width (main_lite.py:80), not the BASELINE config"),
                          "parallelism": f"rays sharded over {world} GPU(s), one all-reduce of the flat gradient arena, BatchNorm statistics "
                                         + ("over the global batch (all-reduced)" if a.bn_sync == "global" and use_dist else "per rank")},
               "final_loss": float(total_of(tot)), "step_ms_median": per_step[len(per_step) // 2], "step_ms_min": per_step[0],
               "per_step_ms": {"median": per_step[len(per_step) // 2], "min": per_step[0], "max": per_step[-1],
                               "note": "stream time of each timed step by HIP events: a hiccup shows as max >> median (ms_per_step is the wall-clock mean)"},
               "host_enqueue_ms_per_step": host_ms, "host_loop_ms_per_step": host_loop_ms,
               "host_note": "host_enqueue = wall time to enqueue one step onto an idle GPU (median of 6; the host's own cost); host_loop = the timed "
                            "loop's enqueue time per step (contains waits for the GPU once the host is ~5 steps ahead)",
               "collectives": dict(sn.parallel.COLLECTIVES) if use_dist else None,
               "roofline": None,
               "step_roofline": {"bound": "hbm", "achieved": hbm_bytes / dt / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": hbm_bytes / dt / 8e12,
                                 "traffic": traffic if Wt == 256 else None, "bytes_per_step": hbm_bytes, "algorithmic_tflops": (flop / dt / 1e12) if flop else None,
                                 "note": "whole step, not one kernel: train-mode BatchNorm forces a layer-wise design in which every layer is "
                                         "a pass over [393216 x width] fp32 arrays; achieved = bytes that design moves per step (counted from "
                                         "the layer table, DESIGN 5.4) / step time, traffic = HBM bytes per step by the PMC counters, "
                                         "peak = HBM3E 8 TB/s (MI355X_MICROARCH.md); per-kernel times in profiles/*/train_kernel_stats.csv"}}
        if world == 1:
            out["roofline"] = train_dominant_kernel(dev, width=Wt)
        if not a.no_cpu_baseline and world == 1:      # reported at N = 1 only (rank 0)
            from oracle import season_nerf_oracle as orc          # CPU-baseline leg only
            torch.set_num_threads(min(host_cpus(), 32))
            sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in orc.init_weights(Wt, NC, 0, bn_stats="identity").items()}
            n = 512
            dc = {k: v[:n].cpu() for k, v in d.items()}
            rng = np.random.Generator(np.random.PCG64(1))
            st = torch.tensor(np.concatenate([rng.uniform(-1, 1, (n, 2)), np.ones((n, 1))], 1), dtype=torch.float32)
            vv = dc["Sun_Angle"]
            solar = {"Top": st, "Bot": st - 2 * vv / vv[:, 2:], "Sun_Angle": vv}
            t0 = time.perf_counter()
            loss, _ = orc.get_loss_mse(sd, dc, solar, S, 0.03, True, True)
            orc.total_loss(loss).backward()
            tc = time.perf_counter() - t0
            out["cpu_baseline"] = {"value": n * S / tc, "unit": "ray-samples/s", "cores": torch.get_num_threads(), "kind": "port",
                                   "sample": f"one MSE training step (forward both passes + backward) on {n} rays x {S} samples, torch-CPU oracle",
                                   "torch_threads": torch.get_num_threads(), **host_info()}
    if use_dist:
        dist.destroy_process_group()
    return out if rank == 0 else None


def _profile_file(name):
    """Newest committed profile summary of that name (profiles/r<N>/<name> or profiles/r<N>/<letter>_<name>)."""
    import glob
    import re
    c = [f for f in glob.glob(os.path.join(REPO, "profiles", "r*", "*" + name)) if re.fullmatch(r"([a-z]_)?" + re.escape(name), os.path.basename(f))]
    if not c:
        raise FileNotFoundError(name)
    return sorted(c, key=lambda f: (int(os.path.basename(os.path.dirname(f))[1:]), os.path.basename(f)))[-1]


def launcher_selftest(a, world, rank):
    """CPU-only check of the N > 1 start-up path (tests/test_parallel_gloo.py): every rank joins a gloo group, one all-reduce,
    rank 0 prints one JSON line.  No GPU, no kernels - it exists so that `python bench.py --gpus N` is exercised where no GPU is."""
    import torch.distributed as dist
    dist.init_process_group("gloo")
    t = torch.tensor([float(rank + 1)])
    dist.all_reduce(t)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"launcher_selftest": True, "n_gpus": world, "backend": "gloo", "rank_sum": float(t.item()),
                          "self_launched": "TORCHELASTIC_RUN_ID" in os.environ}))
    dist.destroy_process_group()


def self_launch(a, argv):
    """`python bench.py --gpus N` with no rank environment: start the N ranks as a child `torch.distributed.run` and exit with
    its status.  Runs BEFORE anything has initialised the GPU in this process (never re-launch from a process that has)."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--prewarm", type=int, default=200, help="untimed steps run before --warmup (reported as `prewarm_steps`): clock ramp of a cold chip; 0 = none")
    ap.add_argument("--prewarm-seconds", type=float, default=2.0, help="the pre-warm lasts at least this long (the part's clock settles over seconds, not over 200 steps)")
    ap.add_argument("--precision", default="auto", choices=["auto", "i8x3", "bf16x3", "bf16"],
                    help="arithmetic of the fused field kernel in the headline timed region (include/season_nerf_hip.h SNERF_PREC_*): "
                         "auto = what season_nerf_amd.T_NeRF picks by default: i8x3 where the pack-time error bound of the int8-digit "
                         "format holds for the weights (it does for the benchmark's init-law weights), else bf16x3; "
                         "i8x3 = 16-bit fixed point on the int8 MFMA pipe (RGB ~1.5e-5 of the reference: inside the 1e-4 bar), "
                         "bf16x3 = 3-term split bf16 products (RGB ~3e-6), bf16 = fast mode, OUTSIDE the bar (RGB 1-3e-3); "
                         "the other modes are timed too and reported under `modes`")
    ap.add_argument("--gather-group", type=int, default=8, help="N > 1: rendered RGB tiles of this many steps share one asynchronous all-gather")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-sweep", action="store_true", help="skip the auxiliary 512x512 sweep measurement (counter passes)")
    ap.add_argument("--workload", default="render", choices=["render", "train"],
                    help="render = headline (BASELINE configs[1]); train = configs[2]: one training step, 4096x96 + 4096 sun rays")
    ap.add_argument("--loss", default="mse", choices=["barron", "mse"], help="colour loss of --workload train (mse = reference-pinned)")
    ap.add_argument("--width", type=int, default=256, choices=[256, 512], help="--workload train: fc_units (256 = BASELINE configs[2]; 512 = the reference's default)")
    ap.add_argument("--headline-only", action="store_true",
                    help="only the headline timed region (no per-mode table, seam, sweep, training step, CPU baseline): profiler passes")
    ap.add_argument("--train-graph", action="store_true", help="--workload train: the step as one hipGraph launch (season_nerf_amd.GraphedTrainStep; one GPU)")
    ap.add_argument("--no-aux", action="store_true", help="render workload: skip the converged-weights rows and the exact-solar pass (kernel-stats passes: they launch the "
                                                        "dominant kernel at other sizes)")
    ap.add_argument("--no-train", action="store_true", help="render workload: skip the extra training-step measurement (train_* keys)")
    ap.add_argument("--train-kernel-only", action="store_true", help="--workload train: only the dominant training kernel (`--steps` launches), for profiler passes")
    ap.add_argument("--aux-kernel", default=None, choices=["sweep", "w512", "w512_bf16x3", "exact_solar", "exact_solar_w512"], help="only that auxiliary kernel, `--steps` launches (profiler passes): "
                                                                              "the seasonal-sweep kernel at 512x512x96, or the W = 512 fused field kernel")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help=argparse.SUPPRESS)   # gloo: CPU test of the launcher only
    ap.add_argument("--bn_sync", default="local", choices=["local", "global"],
                    help="--workload train, N > 1: BatchNorm statistics per rank, or over the global batch (RCCL all-reduces of the "
                         "per-layer statistics: the single-process reference's semantics)")
    ap.add_argument("--full", action="store_true",
                    help="render workload: also measure everything beside the headline (repeated blocks, per-mode table, W = 512 / converged / exact-solar rows, "
                         "512x512 sweep, evaluator seam, training steps, CPU baseline); the --no-* options above then leave parts out. Without it a run "
                         "sets up, warms up, times --steps steps and prints the headline line")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="render workload: after the timed steps write what the last timed step computed (RGB, per-ray class weights and sky colour, "
                         "per-sample density / solar visibility / colour) as DIR/<name>.npy, float32")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if a.dump_outputs and (a.workload != "render" or a.aux_kernel or a.backend == "gloo"):
        ap.error("--dump-outputs applies to the render workload")
    if not a.full and a.workload == "render":          # a plain render run: the headline alone
        a.headline_only = a.no_aux = True
    if a.headline_only:
        a.no_sweep = a.no_train = a.no_cpu_baseline = True
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(a, sys.argv[1:]))          # child ranks; nothing here has touched the GPU
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = _local_device()
    if a.gpus != world and world > 1:
        raise SystemExit(f"--gpus {a.gpus} but the launcher started {world} ranks")
    if a.backend == "gloo":
        return launcher_selftest(a, world, rank)
    if a.aux_kernel:
        torch.cuda.set_device(local)
        dv = torch.device("cuda", local)
        if a.aux_kernel == "sweep":
            print(json.dumps(sweep_kernel_roofline(dv, launches=max(a.steps, 1))))
        elif a.aux_kernel in ("exact_solar", "exact_solar_w512"):
            import season_nerf_amd as sn
            if a.aux_kernel == "exact_solar_w512":            # the reference's default configuration: width 512, converged (sharp) weights -> bf16x3, the K-split kernel
                nx = sn.T_NeRF(512, NC)
                nx.load_state_dict(sharp_state_dict(512)[0])
            else:
                nx = sn.T_NeRF(W, NC)
                nx.load_state_dict(sn.synthetic_state_dict(nx, 0))
            nx.precision = a.precision
            print(json.dumps(exact_solar_bench(dv, nx.to(dv).eval(), sizes=((256, 256, 96),))))
        else:
            import season_nerf_amd as sn
            print(json.dumps(w512_kernel_roofline(dv, synth(0, dv), sn.sample_parameters(S, eval_mode=True).to(dv), launches=max(a.steps, 1),
                                                  precision="bf16x3" if a.aux_kernel == "w512_bf16x3" else "auto")[1]))
        return
    if a.workload == "train" and a.train_kernel_only:        # profiler passes over the dominant training kernel alone
        torch.cuda.set_device(local)
        print(json.dumps(train_dominant_kernel(torch.device("cuda", local), launches=max(a.steps, 1))))
        return
    if a.workload == "train":
        out = bench_train(a)
        if out is not None:
            print(json.dumps(out))
        return
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    use_dist = world > 1 or "RANK" in os.environ          # under torch.distributed.run the RCCL path runs even with one rank
    if use_dist:
        import torch.distributed as dist
        _init_group(dist, dev)

    import season_nerf_amd as sn
    L = sn._lib.lib()
    net = sn.T_NeRF(W, NC)
    net.load_state_dict(sn.synthetic_state_dict(net, 0))   # random weights of the reference's init law, random BatchNorm statistics
    net.precision = a.precision
    net = net.to(dev).eval()
    model = net.device_model()
    prec = net.resolved_precision                          # "auto" resolved: the mode the kernels below run in
    d = synth(rank, dev)
    top, bot, sun, tim = d["Top"], d["Bot"], d["Sun_Angle"], d["Time_Encoded"]
    tv = sn.sample_parameters(S, eval_mode=True).to(dev)
    e = lambda *s: torch.empty(*s, device=dev)
    cls, sky_raw, sky = e(R, NC), e(R, 3), e(R, 3)
    rho, sv, col = e(R * S), e(R * S), e(R * S, 3)
    # RGB tiles of 8 consecutive steps share one asynchronous all-gather on double-buffered tile groups (parallel.TileGroupGather)
    tg = sn.parallel.TileGroupGather((R, 3), group=a.gather_group, device=dev) if use_dist else None
    rgb_local = e(R, 3)
    fo = sn._lib.FieldOut(d_rho=rho.data_ptr(), d_solar_vis=sv.data_ptr(), d_col=col.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev0 = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps)]
    ev1 = [torch.cuda.Event(enable_timing=True) for _ in range(a.steps)]

    def step(i=None):
        sn._lib.check(L.snerf_group_forward(model, R, tim.data_ptr(), sun.data_ptr(), cls.data_ptr(), sky_raw.data_ptr(),
                                            sky.data_ptr(), st), "group")
        if i is not None:
            ev0[i].record()
        sn._lib.check(L.snerf_field_forward_rays(model, 0, R, S, top.data_ptr(), bot.data_ptr(), tv.data_ptr(),
                                                 1, sun.data_ptr(), cls.data_ptr(), C.byref(fo), st), "field")
        if i is not None:
            ev1[i].record()
        out = tg.slot() if use_dist else rgb_local
        co = sn._lib.CompositeOut(d_rgb=out.data_ptr())
        sn._lib.check(L.snerf_composite_rays(R, S, top.data_ptr(), bot.data_ptr(), tv.data_ptr(), rho.data_ptr(),
                                             col.data_ptr(), sv.data_ptr(), sky.data_ptr(), 0, None, 1.0, C.byref(co), st),
                      "composite")
        if use_dist:
            tg.commit()

    # declared, untimed pre-warm BEFORE the driver's --warmup: the chip's clock depends on its load history, and a 20-step sample taken 5 steps
    # after start-up read 8 % slower than the same block repeated right after (round 3: 0.818 against a median of 0.752 ms)
    n_pre, t_pre = 0, time.perf_counter()
    while n_pre < a.prewarm or (a.prewarm > 0 and time.perf_counter() - t_pre < a.prewarm_seconds):      # at least --prewarm steps AND --prewarm-seconds of load
        for _ in range(50):
            step()
        torch.cuda.synchronize()
        n_pre += 50
    for _ in range(a.warmup):
        step()
    if use_dist:
        tg.reset()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(a.steps):
        step(i)
    if use_dist:
        tg.flush()
    if use_dist:
        dist.barrier()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    if use_dist:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt = float(tt.item())
    field_ms = float(np.mean([ev0[i].elapsed_time(ev1[i]) for i in range(a.steps)]))
    if a.dump_outputs and rank == 0:
        # what the last timed step left in its output buffers (nothing below has run yet); under N > 1 the all-gathered RGB of every rank
        os.makedirs(a.dump_outputs, exist_ok=True)
        outs = {"rgb": tg.gathered(a.steps - 1) if use_dist else rgb_local, "class_weights": cls, "sky_color_raw": sky_raw, "sky_color": sky,
                "rho": rho.view(R, S), "solar_vis": sv.view(R, S), "color": col.view(R, S, 3)}
        for k, v in outs.items():
            np.save(os.path.join(a.dump_outputs, k + ".npy"), v.detach().float().cpu().numpy())
    blocks = None
    if rank == 0 and world == 1 and not use_dist and a.full:
        # the same K-step block 25 more times (outside the headline region): one 17 ms sample on a chip whose clock depends on its load
        # history is a thin basis - median and spread of the per-step time go into the line as extra keys
        bl = []
        for _ in range(25):
            torch.cuda.synchronize()
            tb = time.perf_counter()
            for _i in range(a.steps):
                step()
            torch.cuda.synchronize()
            bl.append((time.perf_counter() - tb) / a.steps * 1e3)
        seq = list(bl)
        bl.sort()
        blocks = {"ms_per_step_in_order": seq, "blocks": len(bl), "steps_per_block": a.steps, "ms_per_step_median": bl[len(bl) // 2], "ms_per_step_min": bl[0],
                  "ms_per_step_max": bl[-1], "value_at_median": R * S / (bl[len(bl) // 2] * 1e-3)}

    extra = {}
    if rank == 0 and world == 1 and not a.headline_only:
        # every arithmetic mode on this same batch (outside the timed region): field-kernel time by HIP events on the launch
        # stream, and the deviation of the rendered colour from the bf16x3 mode (itself within ~3e-6 of the reference:
        # tests/test_gpu_parity.py; each mode's own error against the reference goldens: tests/test_gpu_precision.py)
        modes, rgb_ref = {}, None
        for pm in ["bf16x3", "i8x3", "bf16"]:
            netp = net if pm == prec else sn.T_NeRF(W, NC)
            if netp is not net:
                netp.load_state_dict(net.state_dict())
                netp.precision = pm
                netp = netp.to(dev).eval()
            mp = netp.device_model()
            run = lambda: sn._lib.check(L.snerf_field_forward_rays(mp, 0, R, S, top.data_ptr(), bot.data_ptr(), tv.data_ptr(), 1,
                                                                  sun.data_ptr(), cls.data_ptr(), C.byref(fo), st), "field")
            for _ in range(3):
                run()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(50):
                run()
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / 50
            co = sn._lib.CompositeOut(d_rgb=rgb_local.data_ptr())
            sn._lib.check(L.snerf_composite_rays(R, S, top.data_ptr(), bot.data_ptr(), tv.data_ptr(), rho.data_ptr(), col.data_ptr(),
                                                 sv.data_ptr(), sky.data_ptr(), 0, None, 1.0, C.byref(co), st), "composite")
            rgb = rgb_local.double().clone()
            rgb_ref = rgb if rgb_ref is None else rgb_ref
            modes[pm] = {"field_kernel_ms": ms, "ray_samples_per_s_kernel": R * S / (ms * 1e-3),
                           "roofline_frac_algorithmic_of_bf16_peak": FLOP_PER_SAMPLE * R * S / (ms * 1e-3) / PEAK_BF16_DENSE,
                           "rgb_max_rel_dev_vs_bf16x3": float(((rgb - rgb_ref).abs() / rgb_ref.abs().clamp_min(1e-3)).max())}
            del netp
        # the reference's default width (main_lite.py:80), fused on the int8 pipe only: same rays, T_NeRF(512, 4)
        try:
            extra["w512"], extra["w512_roofline"] = w512_kernel_roofline(dev, d, tv)
        except Exception as ex:
            extra["w512_error"] = repr(ex)
        extra["modes"] = modes
        extra["modes_note"] = ("parity bar (north star): RGB / depth within 1e-4 relative of the reference; measured against the reference's "
                               "goldens in tests/: bf16x3 ~3e-6, i8x3 ~1.5e-5 (W=512: 2.5e-5), bf16 1-2e-3 (outside the bar: fast mode only)")
    late = {}      # the rows a reader of the LAST kilobytes of the line must find (the driver keeps an 8 KB tail): emitted after the training block, in front of `roofline`
    if rank == 0 and world == 1 and not a.headline_only and not a.no_aux:
        # converged-weights rows beside the random-weights headline (VERDICT r4 #1c): the same batch with weights that have SURFACES in them
        for wv in (256, 512):
            try:
                late["converged" if wv == 256 else "converged_w512"] = converged_row(dev, d, tv, wv)
            except Exception as ex:
                late[f"converged_w{wv}_error"] = repr(ex)
        try:      # the reference's default width in the arithmetic a converged checkpoint gets (round 6: the K-split kernel), field kernel alone
            late["w512_bf16x3"], late["w512_bf16x3_roofline"] = w512_kernel_roofline(dev, d, tv, precision="bf16x3")
        except Exception as ex:
            late["w512_bf16x3_error"] = repr(ex)
        try:      # the exact-solar pass (the default of both reference renderers), on the headline network and on the sharp one
            late["exact_solar"] = exact_solar_bench(dev, net)
            sd_s, _, _ = sharp_state_dict(256)
            ns = sn.T_NeRF(W, NC)
            ns.load_state_dict(sd_s)
            ns = ns.to(dev).eval()
            late["exact_solar_converged"] = exact_solar_bench(dev, ns, sizes=((256, 256, 96),))
            late["renderer_a_converged"] = renderer_a_row(dev, ns)
            del ns
        except Exception as ex:
            late["exact_solar_error"] = repr(ex)
        try:      # ... at the reference's DEFAULT width (main_lite.py:80; exact solar on is the default of both renderers): init-law weights (auto -> int8 digits) and
            # the sharp set (auto -> bf16x3, the K-split kernel), the latter with the layer-wise composition it replaced timed beside it
            n5 = sn.T_NeRF(512, NC)
            n5.load_state_dict(sn.synthetic_state_dict(n5, 0))
            late["exact_solar_w512"] = exact_solar_bench(dev, n5.to(dev).eval(), sizes=((256, 256, 96),))
            del n5
            sd5, _, _ = sharp_state_dict(512)
            n5 = sn.T_NeRF(512, NC)
            n5.load_state_dict(sd5)
            n5 = n5.to(dev).eval()
            late["exact_solar_converged_w512"] = exact_solar_bench(dev, n5, sizes=((256, 256, 96),), layerwise_too=True)
            late["renderer_a_converged_w512"] = renderer_a_row(dev, n5)
            del n5
        except Exception as ex:
            late["exact_solar_w512_error"] = repr(ex)
    if rank == 0 and world == 1 and not a.no_sweep:
        # outside the timed region: a whole 512x512x96 novel-view image and the 12-step seasonal sweep (BASELINE configs[4],
        # single GPU), through the renderer seam (component render + sweep kernel); wall clock incl. host-side ray grid
        WC, H4 = np.array([41.29, -95.9, 300.0]), np.array([[310.0, 12.0, 0.0, -11650.0], [-9.0, 240.0, 0.0, 23390.0], [0.0, 0.0, 0.01, -3.0], [0, 0, 0, 1.0]])
        try:
            t_sweep = float("inf")
            for rep in range(4):                 # first call warms up allocations; best of the next three (host-side ray grid included)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                img = sn.render_season_sweep(net, (80, 0), (30, 90), [k / 12.0 for k in range(12)], (512, 512, S), WC, H4, dev)
                torch.cuda.synchronize()
                if rep:
                    t_sweep = min(t_sweep, time.perf_counter() - t1)
            extra.update({"image_512x512x96_12step_sweep_ms": t_sweep * 1e3, "sweep_output_shape": list(img.shape)})
            del img
            extra["sweep_roofline"] = sweep_kernel_roofline(dev)
        except Exception as ex:      # never let the auxiliary measurement break the headline line
            extra["image_sweep_error"] = repr(ex)

    if rank == 0 and world == 1 and not a.headline_only:
        # the same batch through the evaluator seam (All_in_One_Eval.eval: allocates its result tensors, returns the whole
        # per-sample dict) - what a reference caller pays per call on top of the raw C-ABI step above
        from types import SimpleNamespace
        eargs = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=True, Use_Solar=True, sc_lambda=0.03,
                                number_low_frequency_cases=NC)
        ev_seam = sn.All_in_One_Eval(eargs, dev, 10, False, None, np.eye(4), np.zeros(3))
        with torch.no_grad():
            for _ in range(3):
                ev_seam.eval(d, net, 0, False)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            n_seam = 50
            for _ in range(n_seam):
                res = ev_seam.eval(d, net, 0, False)
            torch.cuda.synchronize()
            extra["eval_seam_ms"] = (time.perf_counter() - t1) / n_seam * 1e3
            extra["eval_seam_note"] = "All_in_One_Eval.eval(data_dict on the GPU, net, 0, False): full 14-key result dict, wall clock per call"
            del res
            # what a parameter change costs the next inference call (an in-loop validation render during training pays it once per
            # save point): state_dict D2H, host-side BatchNorm fold + error model + fragment packing, H2D upload
            tp = []
            for _ in range(3):
                net.invalidate_packed()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                net.device_model()
                torch.cuda.synchronize()
                tp.append((time.perf_counter() - t1) * 1e3)
            extra["repack_ms"] = min(tp)
            net._probe_memo = None                   # ... and with the measured second stage of `auto` (the int8-vs-bf16x3 probe renders) not reused from the last pack
            net.invalidate_packed()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            net.device_model()
            torch.cuda.synchronize()
            extra["repack_with_probe_ms"] = (time.perf_counter() - t1) * 1e3
            extra["repack_note"] = "T_NeRF.device_model() after a parameter change: D2H of the state_dict + host pack (fold, int8 error model, digits) + upload"
        if not a.no_train:
            del rho, sv, col
            import gc
            gc.collect()                 # the networks / engines of the rows above are cyclic garbage: collected HERE, not inside the timed steps below
            torch.cuda.empty_cache()
            try:
                tr = bench_train(argparse.Namespace(**{**vars(a), "loss": "mse"}), standalone=False)
                extra.update({"train_ms_per_step": tr["ms_per_step"], "train_value": tr["value"], "train_unit": tr["unit"],
                              "train_metric": tr["metric"], "train_steps": tr["steps"], "train_final_loss": tr["final_loss"],
                              "train_dtype": tr["dtype"], "train_roofline": tr["roofline"], "train_step_roofline": tr["step_roofline"],
                              "train_config": tr["config"], "train_per_step_ms": tr["per_step_ms"]})
                extra["train_host_enqueue_ms_per_step"] = tr["host_enqueue_ms_per_step"]
                extra["train_host_note"] = tr["host_note"]
                if "cpu_baseline" in tr:
                    extra["train_cpu_baseline"] = tr["cpu_baseline"]
            except Exception as ex:      # never let the auxiliary measurement break the headline line
                extra["train_error"] = repr(ex)
            try:      # the same MSE step replayed as ONE hipGraph launch per step (season_nerf_amd.GraphedTrainStep): what the host costs then
                torch.cuda.empty_cache()
                tg_ = bench_train(argparse.Namespace(**{**vars(a), "loss": "mse", "train_graph": True, "no_cpu_baseline": True}), standalone=False)
                extra.update({"train_graph_ms_per_step": tg_["ms_per_step"], "train_graph_host_enqueue_ms_per_step": tg_["host_enqueue_ms_per_step"],
                              "train_graph_final_loss": tg_["final_loss"], "train_graph_per_step_ms": tg_["per_step_ms"],
                              "train_graph_note": "the eager step above captured once and replayed as one hipGraph per step; per step the host draws the jitter "
                                                  "vectors and the random sun rays (host RNG, the reference's order), uploads them and Adam's scalars, launches the graph"})
            except Exception as ex:
                extra["train_graph_error"] = repr(ex)
            try:      # configs[2] names the Barron loss: the same step with the adaptive loss object + its own Adam (PARITY UNPINNED)
                torch.cuda.empty_cache()
                tb = bench_train(argparse.Namespace(**{**vars(a), "loss": "barron", "no_cpu_baseline": True}), standalone=False)
                extra.update({"train_barron_ms_per_step": tb["ms_per_step"], "train_barron_final_loss": tb["final_loss"], "train_barron_per_step_ms": tb["per_step_ms"],
                              "train_barron_host_enqueue_ms_per_step": tb["host_enqueue_ms_per_step"],
                              "train_barron_note": "same step with the Barron adaptive colour loss (configs[2] names it) and its second Adam; the loss "
                                                   "object restates robust_loss_pytorch from its published definition: parity UNPINNED (no importable "
                                                   "reference, no reference-held fixture) - a timing, not a reference-checked result"})
            except Exception as ex:
                extra["train_barron_error"] = repr(ex)
            try:      # ... and that step captured: the generic loss terms, both Adams (the second in torch's capturable form) in one hipGraph launch
                gc.collect()
                torch.cuda.empty_cache()
                tbg = bench_train(argparse.Namespace(**{**vars(a), "loss": "barron", "train_graph": True, "no_cpu_baseline": True}), standalone=False)
                extra.update({"train_barron_graph_ms_per_step": tbg["ms_per_step"], "train_barron_graph_host_enqueue_ms_per_step": tbg["host_enqueue_ms_per_step"],
                              "train_barron_graph_final_loss": tbg["final_loss"], "train_barron_graph_per_step_ms": tbg["per_step_ms"]})
            except Exception as ex:
                extra["train_barron_graph_error"] = repr(ex)
            try:      # the reference's DEFAULT width (main_lite.py:80, fc_units = 512), MSE loss
                torch.cuda.empty_cache()
                t5 = bench_train(argparse.Namespace(**{**vars(a), "loss": "mse", "width": 512, "no_cpu_baseline": True}), standalone=False)
                extra.update({"train_w512_ms_per_step": t5["ms_per_step"], "train_w512_value": t5["value"], "train_w512_roofline": t5["roofline"],
                              "train_w512_config": t5["config"], "train_w512_host_enqueue_ms_per_step": t5["host_enqueue_ms_per_step"],
                              "train_w512_per_step_ms": t5["per_step_ms"]})
            except Exception as ex:
                extra["train_w512_error"] = repr(ex)

    if rank == 0:
        value = world * R * S * a.steps / dt
        achieved = FLOP_PER_SAMPLE * R * S / (field_ms * 1e-3)
        traffic = None          # HBM bytes per launch from the committed PMC passes of this same command (profiles/): int8-digit kernel only
        try:
            tj = json.load(open(_profile_file("traffic.json")))
            if prec == "i8x3" and "i8" in tj.get("kernel", ""):
                traffic = tj["bytes_per_launch"]
        except Exception:
            pass
        out = {
            "metric": "ray-samples/sec (4096 rays x 96 samples forward render, T_NeRF 8x256)",
            "value": value, "unit": "ray-samples/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "prewarm_steps": n_pre,
            "ms_per_step": dt / a.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": DTYPES[prec], "precision": a.precision, "precision_resolved": prec, "data": "synthetic",
            "config": {"workload": "BASELINE configs[1]: forward render 4096 rays x 96 samples, T_NeRF(256,4) eval-mode, "
                                   "random weights (reference init law), per-ray sun/time", "rays_per_gpu": R,
                       "samples_per_ray": S, "parallelism": f"rays sharded over {world} GPU(s), RGB tiles all-gathered ({a.gather_group} steps per collective, asynchronous)"},
            "per_gpu_value": value / world, "collectives": dict(sn.parallel.COLLECTIVES) if use_dist else None,
            "image_512x512x96_ms_est": 512 * 512 * S / (value / world) * 1e3, "repeat": blocks,
            "i8_estimate": ({k: v for k, v in net.i8_estimate().items() if k in ("rgb_pred", "budget", "acc_bound", "ok")} if W in (64, 256, 512) else None), **extra, **late,
            # `frac` is priced against the dense peak of the pipe the kernel issues on (int8 digits: 5 Pop/s); the bf16 figure the north star names is beside it
            "roofline": {"bound": "mfma", "achieved": achieved / 1e12, "peak": (PEAK_INT8_DENSE if prec == "i8x3" else PEAK_BF16_DENSE) / 1e12, "unit": "TFLOP/s",
                         "frac": achieved / (PEAK_INT8_DENSE if prec == "i8x3" else PEAK_BF16_DENSE), "frac_of_bf16_peak": achieved / PEAK_BF16_DENSE, "traffic": traffic,
                         "kernel": KERNELS[prec], "kernel_ms": field_ms,
                         "executed_tops": MFMAS_PER_WAVE_TILE[prec] * 65536 * (R * S / 32) / (field_ms * 1e-3) / 1e12,
                         # measured, not nominal: back-to-back int8 MFMAs whose operands change every instruction hold 1.60 GHz on this part = 3.35 POP/s
                         # (tools/probes/wave_spec_i8.hip "MFMA-live", profiles/r4/wave_spec_i8_probe.txt; constant operands: 2.10 GHz); an extra, `frac` is unchanged
                         "executed_frac_of_sustained_int8_rate": (MFMAS_PER_WAVE_TILE[prec] * 65536 * (R * S / 32) / (field_ms * 1e-3) / 3.35e15) if prec == "i8x3" else None,
                         "note": "achieved = algorithmic 1.489 MFLOP/ray-sample x 393216 / kernel time; peak = the dense MFMA peak of the kernel's own dtype "
                                 "(int8: 5 Pop/s = 2x bf16 per clock; MI355X_MICROARCH.md), frac_of_bf16_peak = against the 2.5 PFLOP/s of the north star's dtype. " + EXEC_NOTE[prec]},
        }
        if not a.no_cpu_baseline and world == 1:      # reported at N = 1 only (rank 0)
            out["cpu_baseline"] = cpu_baseline()
        print(json.dumps(out))
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
