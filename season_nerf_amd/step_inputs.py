"""What a training step draws per step besides its batch, drawn on the device: the random sun rays of the solar-correction loss
(`create_solor_rays_uniform`, Eval_Tools_2.py:72-108), the jitter of both sampling passes (`sample_parameters`, misc.py:236-241) and one row of a schedule
table - Adam's six scalars, the DSM prior's trust factor, the second optimiser's learning rate.  One HIP kernel plus a one-thread advance kernel
(csrc/loader.hip); the position {draws, step} lives in device memory behind the C handle, so a captured step that begins with the draw
(`GraphedTrainStep(tool, loader=..., inputs="device")`) takes no host input at all between two replays.

    inputs = DeviceStepInputs(tool, n_rays, n_samples, seed=0)
    out = inputs.draw()                         # nine device tensors: starts, ends, vec, times, tv_image, tv_solar, hyper, trust, lr2
    ref = inputs.host_mirror(draws=0)           # the same nine as numpy arrays, no GPU needed

The law is the host path's, the numbers are not: the stream is Philox4x32-10 under a key of its own (word assignment: csrc/loader_common.h), resumable
(`state_dict`) and rank-aware.  The host statement of the sun-ray law is `training.solar_rays_from_uniforms` - the one function the host generator uses too."""
import ctypes as C
import warnings

import numpy as np
import torch

from . import _lib

NAMES = ("starts", "ends", "vec", "times", "tv_image", "tv_solar", "hyper", "trust", "lr2")
_OP_ORDER = ("starts", "ends", "vec", "times", "base", "tv_image", "tv_solar", "hyper", "trust", "lr2")
MAX_RANK = 1 << 24


def host_words(seed, draws, rank, n_rays, n_samples):
    """The raw 32-bit words of draw `draws` on `rank`: (ray_words [n_rays, 8], sample_words [n_samples, 4]) uint32, computed on the host."""
    rw, sw = np.zeros((n_rays, 8), dtype=np.uint32), np.zeros((n_samples, 4), dtype=np.uint32)
    _lib.check(_lib.lib().snerf_step_inputs_words_host(int(seed) & (2 ** 64 - 1), int(draws), int(rank), n_rays, n_samples, rw.ctypes.data, sw.ctypes.data),
               "snerf_step_inputs_words_host")
    return rw, sw


def _u24(words):
    """u in [0, 1) from the top 24 bits, exact in fp32 (loader_uniform of csrc/loader_common.h)."""
    return (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def host_uniforms(seed, draws, rank, n_rays, n_samples):
    """The uniforms of one draw by name: az, el (float64, all 32 bits), x, y, t0, t1, jitter_image, jitter_solar (fp32, top 24 bits)."""
    rw, sw = host_words(seed, draws, rank, n_rays, n_samples)
    return {"az": rw[:, 0].astype(np.float64) * 2.0 ** -32, "el": rw[:, 1].astype(np.float64) * 2.0 ** -32, "x": _u24(rw[:, 2]), "y": _u24(rw[:, 3]),
            "t0": _u24(rw[:, 4]), "t1": _u24(rw[:, 5]), "jitter_image": _u24(sw[:, 0]), "jitter_solar": _u24(sw[:, 1])}


def jitter_base(n_samples):
    """linspace(0, 1, S + 1)[:-1] with torch's CPU op, as `sample_parameters` builds it: fp32 numpy."""
    return torch.linspace(0, 1, n_samples + 1)[0:-1].float().contiguous().numpy()


def schedule_table(lr, total_steps, lr_alpha_scale=1.0, n_steps_total=1, first_step=0, betas=(0.9, 0.999), eps=1e-8):
    """[total_steps, 8] fp32: row k = what Adam step k + 1 of a phase reads - [lr, b1, b2, eps, 1 - b1^(k+1), 1 - b2^(k+1)] with the OneCycle learning rate after
    k scheduler steps (Net_tool._build_optimisers' schedule, stepped on a throwaway optimiser: the host path's values bit for bit), the DSM prior's trust
    factor (first_step + k) / n_steps_total, and the second optimiser's learning rate (lr * lr_alpha_scale under its own OneCycle)."""
    def lrs(max_lr):
        opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=max_lr)
        sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=max_lr, total_steps=total_steps, base_momentum=0.85, max_momentum=0.95, cycle_momentum=False)
        out = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")             # (scheduler stepped without optimiser steps: nothing is being optimised here)
            for k in range(total_steps):
                out.append(float(opt.param_groups[0]["lr"]))
                if k + 1 < total_steps:
                    sched.step()
        return out
    total_steps = int(total_steps)
    b1, b2 = betas
    tab = np.zeros((total_steps, 8), dtype=np.float64)
    tab[:, 0], tab[:, 7] = lrs(lr), lrs(lr * lr_alpha_scale)
    tab[:, 1], tab[:, 2], tab[:, 3] = b1, b2, eps
    tab[:, 4] = [1.0 - b1 ** (k + 1) for k in range(total_steps)]
    tab[:, 5] = [1.0 - b2 ** (k + 1) for k in range(total_steps)]
    tab[:, 6] = [(first_step + k) / n_steps_total for k in range(total_steps)]
    return tab.astype(np.float32)


class DeviceStepInputs:
    """See the module text.

    tool_or_args   a trainer.Net_tool (matrix and centre of its evaluator, schedule of its optimisers, the prior's phase length), or a mapping / namespace with
                   `W2L_H`, `WC` and optionally `lr`, `total_steps`, `lr_alpha_scale`, `n_steps_total` (no schedule: a table of one zero row)
    rank           < 2^24: ranks draw unrelated streams from one seed
    first_step     the caller's step number of the table's row 0 (enters the trust factor only)
    device         where the draws land (default: the tool's device, else cuda); nothing touches it before the first draw
    """

    def __init__(self, tool_or_args, n_rays, n_samples, seed, rank=0, first_step=0, device=None):
        self.n_rays, self.n_samples, self.seed, self.rank, self.first_step = int(n_rays), int(n_samples), int(seed), int(rank), int(first_step)
        self._handle = None
        self._tool = None
        src = tool_or_args
        if hasattr(src, "eval_tool") and hasattr(src, "optim"):
            ev = src.eval_tool
            H, WC = ev.H, ev.WC
            lr, total, scale = src._schedule
            g = src.optim.param_groups[0]
            self.table_host = schedule_table(lr, total, scale, ev.n_steps, self.first_step, tuple(g["betas"]), g["eps"])
            device = ev.device if device is None else device
            self._tool = src
        else:
            get = src.get if hasattr(src, "get") else (lambda k, d=None: getattr(src, k, d))
            H, WC = get("W2L_H"), get("WC")
            if get("lr") is not None:
                self.table_host = schedule_table(get("lr"), get("total_steps"), get("lr_alpha_scale", 1.0), get("n_steps_total", 1), self.first_step)
            else:
                self.table_host = np.zeros((1, 8), dtype=np.float32)
        self.H = np.ascontiguousarray(np.asarray(H, dtype=np.float64).reshape(4, 4))
        self.WC = np.ascontiguousarray(np.asarray(WC, dtype=np.float64).reshape(3))
        self.device = torch.device("cuda" if device is None else device)
        self.base_host = jitter_base(self.n_samples)
        self._table = self._base = self._op = self.buffers = None
        self._steps = 0                    # rows of the table consumed so far (host count: eager draws + replays of a captured draw)
        self._create(None)

    # -- handle ----------------------------------------------------------------------------------------------------------------
    def _create(self, d_table):
        """(Re)create the C handle over `d_table`; without one (no draw yet) over a placeholder address that is never read - the argument checks run either way."""
        L = _lib.lib()
        state = self._shadow_state() if self._handle else (0, 0, 0, 0)
        self._destroy()
        h = C.c_void_p()
        _lib.check(L.snerf_step_inputs_create(self.seed & (2 ** 64 - 1), self.n_rays, self.n_samples, self.rank, self.H.ctypes.data, self.WC.ctypes.data,
                                              d_table if d_table else self.table_host.ctypes.data, int(self.table_host.shape[0]), C.byref(h)), "snerf_step_inputs_create")
        self._handle, self._on_device = h.value, bool(d_table)
        if any(state):
            self._set(state)

    def _destroy(self):
        if getattr(self, "_handle", None):
            try:
                _lib.lib().snerf_step_inputs_destroy(self._handle)
            except Exception:
                pass
            self._handle = None

    __del__ = _destroy

    def _ensure_device(self):
        if self._on_device:
            return
        from . import ops
        self._op = ops.load().step_inputs_draw
        self._table = torch.from_numpy(self.table_host).to(self.device)
        self._base = torch.from_numpy(self.base_host).to(self.device)
        self._create(self._table.data_ptr())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream) if self._on_device else None

    def _shadow_state(self):
        s = np.zeros(4, dtype=np.int64)
        _lib.check(_lib.lib().snerf_step_inputs_get_state(self._handle, s.ctypes.data, self._stream()), "snerf_step_inputs_get_state")
        return tuple(int(x) for x in s)

    def _set(self, state4):
        s = np.array(state4, dtype=np.int64)
        _lib.check(_lib.lib().snerf_step_inputs_set_state(self._handle, s.ctypes.data, self._stream()), "snerf_step_inputs_set_state")

    # -- drawing ---------------------------------------------------------------------------------------------------------------
    def new_buffers(self):
        e = lambda *sh: torch.empty(*sh, device=self.device)
        R, S = self.n_rays, self.n_samples
        return {"starts": e(R, 3), "ends": e(R, 3), "vec": e(R, 3), "times": e(R, 4), "tv_image": e(S), "tv_solar": e(S), "hyper": e(6), "trust": e(1), "lr2": e(())}

    def draw_into(self, buffers):
        """Draw into caller-owned device tensors: `buffers` maps names of NAMES to float32 tensors of that output's size; names that are missing (or None) are
        not produced.  Safe inside a stream capture once one draw has run eagerly (the first draw allocates the state)."""
        unknown = set(buffers) - set(NAMES)
        if unknown:
            raise ValueError(f"DeviceStepInputs.draw_into: unknown outputs {sorted(unknown)}")
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            if self._steps >= self.table_host.shape[0] and any(buffers.get(k) is not None for k in ("hyper", "trust", "lr2")):
                raise ValueError(f"DeviceStepInputs: step {self._steps} is past the schedule's {self.table_host.shape[0]} rows")
            self._ensure_device()
        elif not self._on_device:
            raise RuntimeError("DeviceStepInputs: draw once eagerly before capturing (the first draw uploads the table and allocates the state)")
        args = [self._base if k == "base" else buffers.get(k) for k in _OP_ORDER]
        self._op(self._handle, self._table, *args)
        if not capturing:
            self._steps += 1

    def note_replay(self):
        """A graph that captured `draw_into` was replayed once: keeps the host's count of consumed schedule rows; refuses past the table's end."""
        if self._steps >= self.table_host.shape[0]:
            raise ValueError(f"DeviceStepInputs: step {self._steps} is past the schedule's {self.table_host.shape[0]} rows")
        self._steps += 1

    def draw(self):
        """The nine outputs of the next draw in fresh device tensors."""
        out = self.new_buffers()
        self.draw_into(out)
        return out

    def __call__(self, n=None, include_times=True):
        """As `create_solor_rays_uniform(...)(n, include_times=True)`: the sun rays of the next draw, device tensors (az / el are not materialised: None)."""
        if n is not None and int(n) != self.n_rays:
            raise ValueError(f"DeviceStepInputs: built for {self.n_rays} rays, asked for {n}")
        e = lambda *sh: torch.empty(*sh, device=self.device)
        out = {"starts": e(self.n_rays, 3), "ends": e(self.n_rays, 3), "vec": e(self.n_rays, 3)}
        if include_times:
            out["times"] = e(self.n_rays, 4)
        self.draw_into(out)
        return (out["starts"], out["ends"], out["vec"]) + ((out["times"], None) if include_times else ())

    # -- position --------------------------------------------------------------------------------------------------------------
    def get_state(self):
        """(draws, step) - read from the device once a draw has run (synchronises the current stream)."""
        return self._shadow_state()[:2]

    def set_state(self, draws, step):
        self._set((int(draws), int(step), 0, 0))
        self._steps = int(step)

    def state_dict(self):
        return {"seed": self.seed, "rank": self.rank, "state": list(self._shadow_state())}

    def load_state_dict(self, state):
        """Continue the stream where `state` was taken (same seed and rank, or the draws that follow would be another stream's)."""
        if int(state["seed"]) != self.seed or int(state["rank"]) != self.rank:
            raise ValueError(f"DeviceStepInputs.load_state_dict: the state belongs to seed {state['seed']} rank {state['rank']}, this object has seed {self.seed} rank {self.rank}")
        self._set(tuple(int(x) for x in state["state"]))
        self._steps = int(state["state"][1])

    # -- host mirror -----------------------------------------------------------------------------------------------------------
    def host_mirror(self, draws, step=None):
        """The nine arrays of draw number `draws` (schedule row `step`, default `draws`; past the end: the last row) as numpy, without a GPU.  Integer words, the
        fp32 outputs of fp32 arithmetic (starts, both jitter vectors) and the table row are the device's bit for bit; vec / ends / times round a float64 value
        whose last bits depend on the libm at hand."""
        from .training import solar_rays_from_uniforms
        u = host_uniforms(self.seed, draws, self.rank, self.n_rays, self.n_samples)
        starts, ends, vec, times, az_el = solar_rays_from_uniforms(np.stack([u["az"], u["el"]], 1), u["x"], u["y"], np.stack([u["t0"], u["t1"]], 1), self.H, self.WC,
                                                                   times_in_float64=True)
        inv_s = np.float32(1.0 / self.n_samples)
        row = self.table_host[min(max(int(draws if step is None else step), 0), self.table_host.shape[0] - 1)]
        return {"starts": starts, "ends": ends, "vec": vec, "times": times, "tv_image": self.base_host + inv_s * u["jitter_image"],
                "tv_solar": self.base_host + inv_s * u["jitter_solar"], "hyper": row[:6].copy(), "trust": row[6:7].copy(), "lr2": row[7:8].copy(), "az_el": az_el}

    # -- serving a Net_tool ----------------------------------------------------------------------------------------------------
    def attach(self, tool):
        """Make `tool` (trainer.Net_tool) take its per-step inputs from this object: its optimisers switch to the form that reads their scalars from device
        memory, `tool.train_step` then starts with one draw.  Returns self."""
        from .trainer import GraphedTrainStep
        if not tool.fused_adam:
            raise ValueError("DeviceStepInputs.attach: needs the fused Adam (its scalars live in device memory)")
        if tool.optim.hyper is None:       # (FusedAdam.make_capturable's vector; the parameter store it asks for the device may not exist before the first step)
            tool.optim.hyper = torch.zeros(6, device=self.device)
        tool.optim.hyper_from_device = True
        if tool.optim2 is not None:
            GraphedTrainStep._torch_adam_capturable(tool.optim2, self.device)
        if self.buffers is None:
            self.buffers = self.new_buffers()
        tool.device_inputs = self
        return self

    def step_buffers(self, tool):
        """The buffers of one training step of `tool`: this object's ray and jitter tensors + the optimisers' own scalars."""
        b = dict(self.buffers, hyper=tool.optim.hyper, lr2=tool.optim2.param_groups[0]["lr"] if tool.optim2 is not None else None)
        if not tool.eval_tool.use_prior:
            b["trust"] = None
        return b

    def check_step(self, current_step):
        if int(current_step) != self.first_step + self._steps:
            raise ValueError(f"DeviceStepInputs: the caller is at step {current_step}, the device schedule at {self.first_step} + {self._steps} "
                             "(the trust factor and the learning rates are read from the table row of the device's own step count)")
