"""step_inputs.DeviceStepInputs on the GPU: the draw kernel against the host mirror, the position in device memory (state, resume, a captured draw), the custom
op, and training through GraphedTrainStep(tool, loader=..., inputs="device") / Net_tool with device inputs attached.

Device against mirror.  Integer words, fp32-only arithmetic (starts, both jitter vectors) and the copied table row must agree bit for bit.  vec, ends and times
round a float64 value to fp32 on both sides; the float64 values differ only in the last bits that two math libraries give cos / sin / tan, so the fp32 results
can differ only where such a value sits on a rounding boundary, and then by one fp32 step of the operands: 2^-23 absolute for vec and times (|value| <= 1),
2^-23 (|start| + |2 vec_c / vec_z|) for ends.  Float64 against extended precision of the same formula disagrees in 1.2e-4 of the vec elements and 4.5e-5 of the
ends elements; fp32 trigonometry on the device would disagree in about 17 % of the times - the cap on the share of elements that differ at all is 1e-3."""
import glob
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_step_inputs_host import H_GEO, H_LOADER, MATRICES, WC

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT, GAP = -7777.0, 64
EPS = 2.0 ** -23
SCHED = dict(lr=3e-4, total_steps=7, lr_alpha_scale=30.0, n_steps_total=40)


def _inputs(H, R, S, seed, **kw):
    import season_nerf_amd as sn
    return sn.DeviceStepInputs(dict(SCHED, W2L_H=H, WC=WC), R, S, seed, **kw)


class Arena:
    """The nine outputs as views of ONE flat tensor, a sentinel gap in front of, between and behind them."""

    def __init__(self, R, S):
        self.sizes = {"starts": (R, 3), "ends": (R, 3), "vec": (R, 3), "times": (R, 4), "tv_image": (S,), "tv_solar": (S,), "hyper": (6,), "trust": (1,), "lr2": ()}
        n = GAP + sum(int(np.prod(s)) + GAP for s in self.sizes.values())
        self.flat = torch.full((n,), SENT, device="cuda")
        self.bufs, self.span, off = {}, {}, GAP
        for k, s in self.sizes.items():
            m = int(np.prod(s))
            self.bufs[k], self.span[k] = self.flat[off:off + m].view(s), (off, off + m)
            off += m + GAP

    def check(self, di, mirror, skipped=()):
        """Everything outside the outputs that were asked for still holds the sentinel; the outputs against the mirror."""
        flat = self.flat.cpu().numpy()
        mask = np.ones(flat.size, dtype=bool)
        for k, (a, b) in self.span.items():
            if k not in skipped:
                mask[a:b] = False
        assert np.all(flat[mask] == np.float32(SENT)), "a write outside the outputs asked for"
        got = {k: flat[a:b].reshape(self.sizes[k] or (1,)) for k, (a, b) in self.span.items() if k not in skipped}
        for k in ("tv_image", "tv_solar", "starts", "hyper", "trust", "lr2"):
            if k in got:
                assert got[k].tobytes() == mirror[k].tobytes(), k
        for k in ("vec", "times"):
            if k in got:
                assert np.abs(got[k].astype(np.float64) - mirror[k]).max() <= EPS, k
        if "ends" in got:
            v = mirror["vec"].astype(np.float64)
            bound = EPS * (np.abs(mirror["starts"].astype(np.float64)) + np.abs(2 * v / v[:, 2:]))
            assert np.all(np.abs(got["ends"].astype(np.float64) - mirror["ends"]) <= bound)
            assert np.all(got["ends"][:, 2] == -1)


@pytest.mark.parametrize("name", list(MATRICES))
@pytest.mark.parametrize("S", [1, 33, 96])
@pytest.mark.parametrize("R", [1, 63, 257, 1000])
def test_device_draws_equal_the_host_mirror(R, S, name):
    """Three consecutive draws that cross the 32-bit boundary of the draw counter, schedule rows 4..6 of 7."""
    di = _inputs(MATRICES[name], R, S, seed=R * 131 + S, rank=5)
    d0 = 2 ** 32 - 2
    di.set_state(d0, 4)
    for j in range(3):
        ar = Arena(R, S)
        di.draw_into(ar.bufs)
        ar.check(di, di.host_mirror(d0 + j, step=4 + j))
        assert di.get_state() == (d0 + j + 1, 5 + j)
    with pytest.raises(ValueError, match="past the schedule"):
        di.draw_into(Arena(R, S).bufs)                        # row 7 of 7: refused on the host, as OneCycleLR refuses its step past the end
    assert di.get_state() == (d0 + 3, 7)


def test_null_outputs_are_skipped():
    di = _inputs(H_LOADER, 257, 33, seed=9)
    for keep in (("starts",), ("ends",), ("vec", "tv_solar"), ("times", "hyper"), ("tv_image", "lr2", "trust"), ()):
        ar = Arena(257, 33)
        d, s = di.get_state()
        di.draw_into({k: (v if k in keep else None) for k, v in ar.bufs.items()})
        ar.check(di, di.host_mirror(d, step=s), skipped=[k for k in ar.bufs if k not in keep])
    assert di.get_state() == (6, 6)
    with pytest.raises(ValueError, match="unknown"):
        di.draw_into({"Top": None})
    st, en, ve, ti, none = di(257, include_times=True)           # the generator's call signature: device tensors of the next draw
    m = di.host_mirror(6)
    assert none is None and st.is_cuda and st.cpu().numpy().tobytes() == m["starts"].tobytes() and ti.shape == (257, 4) and len(di(257)) == 5


def test_share_of_elements_that_differ_from_the_mirror_at_all():
    R = 100003
    di = _inputs(H_GEO, R, 96, seed=77)
    out, m = di.draw(), di.host_mirror(0)
    for k in ("starts", "tv_image", "tv_solar"):
        assert out[k].cpu().numpy().tobytes() == m[k].tobytes(), k
    for k in ("vec", "ends", "times"):
        got = out[k].cpu().numpy()
        share = float((got != m[k]).mean())
        print(f"  {k}: share of elements that differ from the mirror {share:.2e}, largest difference {np.abs(got.astype(np.float64) - m[k]).max():.3e}")
        assert share <= 1e-3, (k, share)


def test_state_resume_and_state_dict():
    a, b = _inputs(H_LOADER, 63, 33, seed=4), _inputs(H_LOADER, 63, 33, seed=4)
    outs = [a.draw() for _ in range(5)]
    assert a.get_state() == (5, 5)
    for k in range(1, 6):
        c = _inputs(H_LOADER, 63, 33, seed=4)
        for _ in range(k):
            c.draw()
        assert c.get_state() == (k, k) and c._steps == k                    # after k draws the device copy equals the host's count
    b.set_state(3, 3)                                                       # resume mid-run
    for j in (3, 4):
        o = b.draw()
        assert all(torch.equal(o[k], outs[j][k]) for k in o), j
    sd = a.state_dict()
    assert sd == {"seed": 4, "rank": 0, "state": [5, 5, 0, 0]}
    c = _inputs(H_LOADER, 63, 33, seed=4)
    c.draw()                                                                # (its device state exists: load replaces both copies)
    c.load_state_dict(sd)
    x, y = a.draw(), c.draw()
    assert all(torch.equal(x[k], y[k]) for k in x) and c.get_state() == (6, 6)
    d = _inputs(H_LOADER, 63, 33, seed=4)
    d.set_state(9, 2)                                                       # phase change: a new schedule position, the stream runs on
    o, m = d.draw(), a.host_mirror(9, step=2)
    assert o["tv_image"].cpu().numpy().tobytes() == m["tv_image"].tobytes() and o["hyper"].cpu().numpy().tobytes() == m["hyper"].tobytes()


def test_a_captured_draw_advances_at_every_replay():
    di = _inputs(H_LOADER, 257, 33, seed=12)
    ar = Arena(257, 33)
    di.draw(), di.draw()                                                    # (the first draw uploads the table and allocates the state: not for a capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        di.draw_into(ar.bufs)
    assert di.get_state() == (2, 2)                                         # a capture executes nothing
    for j in range(5):
        ar.flat.fill_(SENT)
        graph.replay()
        ar.check(di, di.host_mirror(2 + j))
    assert di.get_state() == (7, 7)


def test_custom_op_under_opcheck():
    import season_nerf_amd as sn
    di, ar = _inputs(H_LOADER, 63, 33, seed=1), Arena(63, 33)
    di.draw()
    order = ("starts", "ends", "vec", "times", "base", "tv_image", "tv_solar", "hyper", "trust", "lr2")
    full = (di._handle, di._table) + tuple(di._base if k == "base" else ar.bufs[k] for k in order)
    torch.library.opcheck(torch.ops.season_nerf.step_inputs_draw.default, full, test_utils=("test_schema", "test_faketensor"))
    some = (di._handle, di._table) + tuple(di._base if k == "base" else (ar.bufs[k] if k in ("vec", "tv_solar") else None) for k in order)
    torch.library.opcheck(torch.ops.season_nerf.step_inputs_draw.default, some, test_utils=("test_schema", "test_faketensor"))
    ops = sn.ops.load()
    with pytest.raises(RuntimeError, match="starts"):
        ops.step_inputs_draw(di._handle, di._table, ar.bufs["starts"][:50], *([None] * 9))
    with pytest.raises(RuntimeError, match="d_base"):
        ops.step_inputs_draw(di._handle, di._table, None, None, None, None, None, ar.bufs["tv_image"], None, None, None, None)
    with pytest.raises(RuntimeError, match="table"):
        ops.step_inputs_draw(di._handle, di._table[:3], *([None] * 10))


# ------------------------------------------------------------------------------------------------------------------ training
W, R, S, N_STEPS, N_TABLE = 64, 96, 32, 8, 1000
CONFIGS = {"mse-free": dict(use_mse=True, prior=False, fused_loss="default", first=0), "barron-prior": dict(use_mse=False, prior=True, fused_loss="all", first=3)}


def _ray_table(rng, n):
    sun = rng.uniform(0.1, 1, (n, 3)); sun /= np.linalg.norm(sun, axis=1, keepdims=True)
    view = rng.uniform(-1, 1, (n, 3)); view /= np.linalg.norm(view, axis=1, keepdims=True)
    tau = rng.uniform(0, 1, (n, 2))
    time = np.stack([np.cos(6.28 * tau[:, 0]), np.sin(6.28 * tau[:, 0]), np.cos(6.28 * tau[:, 1]), np.sin(6.28 * tau[:, 1])], 1)
    return np.concatenate([rng.integers(0, 64, (n, 2)), rng.uniform(-1, 1, (n, 2)), np.ones((n, 1)), rng.uniform(-1, 1, (n, 2)), -np.ones((n, 1)), view, sun, time,
                           np.ones((n, 1)), rng.uniform(0, 1, (n, 3))], 1).astype(np.float32)


class _Counters:
    """Counts what reaches the device from the host inside the training module: uploads through the pinned ring, and _to_dev calls on a host tensor (device
    tensors pass through _to_dev untouched - the capture itself calls it on the graph's own buffers)."""

    def __init__(self, training):
        self.t, self.ring, self.to_dev, self.on = training, 0, 0, False
        self._upload, self._to_dev = training._RING.upload, training._to_dev

    def __enter__(self):
        def upload(t, dev):
            self.ring += int(self.on)
            return self._upload(t, dev)

        def to_dev(t, dev):
            self.to_dev += int(self.on and t.device.type == "cpu")
            return self._to_dev(t, dev)
        self.t._RING.upload, self.t._to_dev = upload, to_dev
        return self

    def __exit__(self, *exc):
        del self.t._RING.upload
        self.t._to_dev = self._to_dev


def _run(config, graphed, inputs):
    import season_nerf_amd as sn
    from oracle import season_nerf_oracle as orc
    from season_nerf_amd import training
    from season_nerf_amd.adaptive_loss import AdaptiveLossFunction
    c = CONFIGS[config]
    tab = torch.from_numpy(_ray_table(np.random.Generator(np.random.PCG64(5)), N_TABLE)).cuda()
    hm = np.random.Generator(np.random.PCG64(3)).uniform(-0.8, 0.6, (24, 24))
    net = sn.T_NeRF(W, 4, HM=hm) if c["prior"] else sn.T_NeRF(W, 4)
    net.load_state_dict(orc.init_weights(W, 4, 7, bn_stats="identity"))
    net = net.cuda().train()
    args = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=False, Use_MSE_loss=c["use_mse"], Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=4)
    mk = lambda dims, a0, s0, slo: AdaptiveLossFunction(dims, torch.float32, "cuda", alpha_hi=2.99, alpha_init=a0, scale_init=s0, scale_lo=slo)
    ada = None if c["use_mse"] else ([mk(3, 2.0, .03, .01), mk(1, 2.0, .5, .05)] if c["prior"] else mk(3, 2.0, .03, .01))
    ev = sn.All_in_One_Eval(args, torch.device("cuda"), 40 if c["prior"] else 10, c["prior"], ada, H_LOADER, WC)
    ev.fused_loss = c["fused_loss"]
    tool = sn.Net_tool(net, ev, 3e-4, total_steps=N_STEPS + 1, lr_alpha_scale=30.0, writer=None)
    ld = sn.DeviceRayLoader(tab, R, seed=21, drop_last=True)
    first = c["first"]
    step = di = None
    if graphed:
        step = sn.GraphedTrainStep(tool, loader=ld, warmup=2, inputs=inputs, seed=31, first_step=first)
        di = step.inputs
    elif inputs == "device":
        di = sn.DeviceStepInputs(tool, R, S, 31, first_step=first).attach(tool)
    assert (di is not None) == (inputs == "device")
    np.random.seed(11); torch.manual_seed(11)
    losses, extra = [], {}
    lr2 = tool.optim2.param_groups[0]["lr"] if (tool.optim2 is not None and inputs == "device") else None
    lr2_ptr = lr2.data_ptr() if lr2 is not None else None
    with _Counters(training) as cnt:
        for k in range(N_STEPS):
            cnt.on = graphed and k >= 2                                     # the six replays
            loss = step(None, first + k) if graphed else tool.train_step(ld.next(), first + k)
            losses.append({n: float(v[0]) for n, v in loss.items()})
    if graphed:
        assert step.graph is not None and step.calls == N_STEPS and not step.disabled
    assert ld.get_state() == (0, N_STEPS, N_STEPS)
    if di is not None:
        assert di.get_state() == (N_STEPS, N_STEPS)
        row = di.table_host[N_STEPS - 1]
        extra["hyper_is_row"] = tool.optim.hyper.cpu().numpy().tobytes() == row[:6].tobytes()
        if lr2 is not None:
            now = tool.optim2.param_groups[0]["lr"]
            extra["lr2_kept"] = torch.is_tensor(now) and now.data_ptr() == lr2_ptr and now.cpu().numpy().tobytes() == row[7].tobytes()
        with pytest.raises(ValueError, match="the caller is at step"):
            (step or tool.train_step)(None if graphed else ld.next(), first + N_STEPS + 5)
    lr_now = tool.sched.get_last_lr()[0]
    return SimpleNamespace(losses=losses, params={k: v.detach().clone() for k, v in net.state_dict().items()}, lr=float(lr_now), ring=cnt.ring, to_dev=cnt.to_dev,
                           extra=extra, adam_steps=net._param_store.adam_steps)


_RUNS = {}


def _cached(config, graphed, inputs):
    key = (config, graphed, inputs)
    if key not in _RUNS:
        _RUNS[key] = _run(*key)
    return _RUNS[key]


def _follows(e, g, label):
    """test_captured_steps_that_draw_inside_the_graph_follow_eager_steps_fed_by_a_loader's tolerances: losses within 2e-4 * max(|v|, 1e-3), parameters within
    0.02 of the distance moved."""
    from oracle import season_nerf_oracle as orc
    assert e.lr == g.lr and e.adam_steps == g.adam_steps == N_STEPS
    for k in range(N_STEPS):
        assert e.losses[k].keys() == g.losses[k].keys()
        for n, v in e.losses[k].items():
            print(f"  {label} step {k} {n}: eager {v:.8e} captured {g.losses[k][n]:.8e}")
            assert abs(g.losses[k][n] - v) <= 2e-4 * max(abs(v), 1e-3), (k, n, g.losses[k][n], v)
    p0 = orc.init_weights(W, 4, 7, bn_stats="identity")
    moved = diff = 0.0
    for k, v in e.params.items():
        if v.is_floating_point() and "running" not in k:
            moved += float((v.cpu() - p0[k]).abs().sum())
            diff += float((g.params[k] - v).abs().sum())
        elif not v.is_floating_point():
            assert torch.equal(g.params[k], v), k
    print(f"  {label}: sum |difference| / sum |update| after {N_STEPS} steps = {diff / moved:.2e}")
    assert moved > 0 and diff < 0.02 * moved, (diff, moved)


@pytest.mark.parametrize("config", list(CONFIGS))
def test_captured_steps_with_device_inputs_follow_eager_steps_fed_by_the_same_stream(config):
    e, g = _cached(config, False, "device"), _cached(config, True, "device")
    _follows(e, g, config)
    assert len({round(l["Color"], 9) for l in g.losses}) == N_STEPS            # eight different batches and draws
    assert len({round(l["Color"], 9) for l in e.losses}) == N_STEPS
    assert g.extra["hyper_is_row"] and e.extra["hyper_is_row"]
    if config == "barron-prior":
        assert g.extra["lr2_kept"] and e.extra["lr2_kept"]                     # written by the kernel only: the tensor of the capture, the table's value


def test_replays_with_device_inputs_take_no_host_input():
    g, h = _cached("mse-free", True, "device"), _cached("mse-free", True, "host")
    print(f"  six replays: ring uploads {g.ring} (host inputs: {h.ring}), _to_dev calls on host tensors {g.to_dev} (host inputs: {h.to_dev})")
    assert g.ring == 0 and g.to_dev == 0
    assert h.ring > 0 and h.to_dev > 0                                         # the control: the same counters see the host path's uploads


def test_host_inputs_behave_as_before():
    """inputs="host" (the default): the captured step's host draws are the eager step's under one numpy / torch seed."""
    e, g = _cached("mse-free", False, "host"), _cached("mse-free", True, "host")
    _follows(e, g, "host inputs")


CHILD = r"""
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import torch
import test_gpu_step_inputs as T
r = T._run("barron-prior", True, "device")
torch.cuda.synchronize()
print("ran", len(r.losses), r.ring, r.to_dev, flush=True)
"""


def test_captured_step_with_device_inputs_holds_kernel_nodes_only(tmp_path):
    """The method of tests/test_gpu_loader_graph_nodes.py (the runtime's own DOT print, in a child process: the switch is read at HIP start-up): not one
    memory-operation node, the loader's two kernels and the two of the step inputs once each."""
    env = dict(os.environ, DEBUG_HIP_GRAPH_DOT_PRINT="1")
    env.pop("SNERF_TRAIN_MEMOPS", None)
    r = subprocess.run([sys.executable, "-c", CHILD % (REPO, REPO)], cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "ran 8 0 0" in r.stdout, r.stdout
    dots = sorted(glob.glob(os.path.join(str(tmp_path), "graph_*dot_print*")))
    assert len(dots) == 1, (dots, r.stderr[-500:])
    labels = re.findall(r'label="\d+\n([^\n"]*)', open(dots[0]).read())
    assert len(labels) > 100, len(labels)
    memops = [l for l in labels if re.search(r"memcpy|memset", l, re.I)]
    assert not memops, f"{len(memops)} memory-operation nodes among {len(labels)}: {sorted(set(memops))}"
    for kernel in ("loader_draw_kernel", "loader_advance_kernel", "step_inputs_draw_kernel", "step_inputs_advance_kernel"):
        assert sum(kernel in l for l in labels) == 1, (kernel, sorted(set(labels))[:40])


def test_net_tool_with_device_inputs_keeps_one_stream_across_phases():
    """T_NeRF_Net_Tool(device_inputs=True): 12 steps - the DSM-prior phase (2 eager steps), then the free phase (2 eager, 8 replays); every step took one draw, the
    phase change rebuilt the table (row 0 = the phase's first step) and kept the draw counter."""
    import season_nerf_amd as sn
    from oracle import season_nerf_oracle as orc
    from test_net_tool import _args
    rng = np.random.Generator(np.random.PCG64(3))
    hm = rng.uniform(-0.8, 0.6, (24, 24))
    train = sn.DeviceRayLoader(torch.from_numpy(_ray_table(rng, 500)).cuda(), 48, seed=1, drop_last=True)
    val = sn.DeviceRayLoader(torch.from_numpy(_ray_table(rng, 200)).cuda(), 48, seed=2)
    tool = sn.T_NeRF_Net_Tool(_args(12, n_saves=3, use_mse=True), hm, hm, "cuda", H_LOADER, WC, train_loader=train, val_loader=val, use_graph=True,
                              device_inputs=True, inputs_seed=5)
    tool.network.load_state_dict(orc.init_weights(64, 4, 1))
    seen = []
    for _ in range(12):
        tool.step()
        seen.append((tool.device_inputs.get_state(), tool.device_inputs.first_step, tool._graphed is not None and tool._graphed.graph is not None))
    assert [s[0][0] for s in seen] == list(range(1, 13))
    assert [s[0][1] for s in seen] == [1, 2] + list(range(1, 11)) and [s[1] for s in seen] == [0, 0] + [2] * 10
    assert [s[2] for s in seen] == [False] * 4 + [True] * 8
    assert all(torch.isfinite(v[0]).all() for v in tool.last_loss.values() if torch.is_tensor(v[0]))
