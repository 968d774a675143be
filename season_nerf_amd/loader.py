"""Device-resident training-data loader: what `Net_tool.get_data` (mg_run_NeRF.py:229-264) assembles per step from two
`DataLoader(shuffle=True, num_workers=4)` objects (mg_run_NeRF.py:74-84; one `__getitem__` per row, NN_loaders/mg_Color_Loader.py:94-102; `t.rand(4)` per
sun-check ray, NN_loaders/mg_SC_loader.py:17-21), `data_to_dict` (:122-133) and the CPU round trip of `get_Dist` (:106-120), drawn by HIP kernels from the
22-column ray table that already lives on the GPU (`raytable.ray_table`).

    loader = DeviceRayLoader(table, batch_size, seed=0, dsm_distance=DSM_Distance(...))
    data = loader.next()                     # the reference's data_dict, device tensors
    tool = T_NeRF_Net_Tool(args, ..., train_loader=loader, val_loader=DeviceRayLoader(val_table, batch_size, seed=1), use_graph=True)

An epoch is a shuffle without replacement - a keyed bijection of the row numbers (Feistel network, cycle-walking) evaluated per element, so no permutation
array exists anywhere - and ends as `DataLoader`'s does (`drop_last=False`: a short last batch).  The position (epoch, batch, draw count) lives in DEVICE
memory behind the C handle: the kernels read it there and a one-thread kernel advances it, so a draw captured in a hipGraph (`next_into` inside
`GraphedTrainStep`) yields a new batch at every replay with no host traffic at all.  The host functions below mirror the integer arithmetic exactly
(`host_indices`, `host_sc_rays`: no GPU needed)."""
import ctypes as C

import numpy as np
import torch

from . import _lib

# name in the data_dict -> (argument position of season_nerf::loader_next after (loader, table), columns)
FIELDS = {"Img_Pt": (0, 2), "Top": (1, 3), "Bot": (2, 3), "View_Angle": (3, 3), "Sun_Angle": (4, 3), "Time_Encoded": (5, 4), "Sample_Weight": (6, 1),
          "GT_Color": (7, 3), "Row_Index": (8, 0), "SC_Top": (9, 3), "SC_Bot": (10, 3)}
_DICT_KEYS = ("Img_Pt", "Top", "Bot", "View_Angle", "Sun_Angle", "Time_Encoded", "Sample_Weight", "GT_Color", "SC_Top", "SC_Bot")


def batches_per_epoch(n_rows, batch_size, drop_last=False, world=1):
    """As len(DataLoader): ceil(N / B), or floor(N / (B * world)) with drop_last."""
    return n_rows // (batch_size * world) if drop_last else -(-n_rows // batch_size)


def epoch_batch_sizes(n_rows, batch_size, drop_last=False, world=1):
    """Row counts of one epoch's batches on every rank (the rule the C handle's host shadow follows)."""
    if drop_last:
        return [batch_size] * batches_per_epoch(n_rows, batch_size, True, world)
    return [min(batch_size, n_rows - k * batch_size) for k in range(batches_per_epoch(n_rows, batch_size))]


def host_indices(n_rows, seed, epoch, first=0, count=None):
    """Positions first .. first + count - 1 of epoch `epoch`'s permutation of range(n_rows): int64 numpy, computed on the host."""
    count = n_rows - first if count is None else count
    out = np.empty(max(count, 0), dtype=np.int64)
    _lib.check(_lib.lib().snerf_loader_indices_host(n_rows, seed, epoch, first, count, out.ctypes.data), "snerf_loader_indices_host")
    return out


def _bounds6(bounds):
    """SC_loader's bounds tensor [[x0, x1], [y0, y1], [z0, z1]] -> six fp32 (None: the cube, setup_SC_loader's default)."""
    if bounds is None:
        return None
    b = np.ascontiguousarray(torch.as_tensor(bounds, dtype=torch.float32).cpu().numpy().reshape(-1))
    if b.size != 6:
        raise ValueError("bounds must be [[x0, x1], [y0, y1], [z0, z1]]")
    return b


def host_sc_rays(seed, draws, rank, first, count, bounds=None):
    """(top, bot) [count, 3] float32 numpy: the sun-check rays first .. first + count - 1 of draw number `draws` on `rank`, computed on the host."""
    b = _bounds6(bounds)
    top, bot = np.empty((count, 3), dtype=np.float32), np.empty((count, 3), dtype=np.float32)
    _lib.check(_lib.lib().snerf_loader_sc_rays_host(seed, draws, rank, first, count, None if b is None else b.ctypes.data, top.ctypes.data, bot.ctypes.data),
               "snerf_loader_sc_rays_host")
    return top, bot


def philox4x32_10(counter, key):
    """The generator behind the sun-check rays (Philox4x32-10): four counter words, two key words -> four uint32."""
    c, k, o = np.asarray(counter, dtype=np.uint32).copy(), np.asarray(key, dtype=np.uint32).copy(), np.zeros(4, dtype=np.uint32)
    if c.size != 4 or k.size != 2:
        raise ValueError("philox4x32_10: counter has 4 words, key 2")
    _lib.check(_lib.lib().snerf_loader_philox_host(c.ctypes.data, k.ctypes.data, o.ctypes.data), "snerf_loader_philox_host")
    return o


class DeviceRayLoader:
    """Shuffled batches of a device-resident [N, 22] ray table; see the module text.

    table         float32 [N, 22] on the GPU (kept, not copied)
    bounds        SC_loader's bounds [[x0, x1], [y0, y1], [z0, z1]] of the random sun-check rays (None: the cube)
    rank, world   data parallel: needs drop_last; the ranks take disjoint consecutive batch_size-blocks of the one permutation
    dsm_distance  a validation.DSM_Distance: next() then also returns Dist_to_Surf_GT / Dist_to_Surf_Prior (get_Dist, mg_run_NeRF.py:263)
    """

    def __init__(self, table, batch_size, seed=0, drop_last=False, bounds=None, rank=0, world=1, dsm_distance=None):
        if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.float32 and table.dim() == 2):
            raise ValueError("DeviceRayLoader: the table is a float32 [N, 22] tensor on the GPU (raytable.ray_table builds one)")
        self.table = table.contiguous()
        self.device = self.table.device
        self.batch_size, self.seed, self.drop_last, self.rank, self.world = int(batch_size), int(seed), bool(drop_last), int(rank), int(world)
        self.n_rows = int(self.table.shape[0])
        self.dsm_distance = dsm_distance
        self._bounds = _bounds6(bounds)
        self._handle = None
        from . import ops
        self._op = ops.load().loader_next
        h = C.c_void_p()
        L = _lib.lib()
        _lib.check(L.snerf_loader_create(self.table.data_ptr(), self.n_rows, int(self.table.shape[1]), self.batch_size, self.seed & (2 ** 64 - 1), int(self.drop_last),
                                         self.rank, self.world, None if self._bounds is None else self._bounds.ctypes.data, C.byref(h)), "snerf_loader_create")
        self._handle = h.value
        self.batches_per_epoch = int(L.snerf_loader_batches_per_epoch(self._handle))
        self._sizes = epoch_batch_sizes(self.n_rows, self.batch_size, self.drop_last, self.world)
        self._batch = 0            # batch_in_epoch of the next EAGER draw: sizes a short last batch (the C handle's shadow follows the same rule)
        self._solar_vecs = None

    def __del__(self):
        if getattr(self, "_handle", None):
            try:
                _lib.lib().snerf_loader_destroy(self._handle)
            except Exception:
                pass
            self._handle = None

    def __len__(self):
        return self.batches_per_epoch

    @property
    def graph_safe(self):
        """Every batch has batch_size rows: the draw may be captured in a hipGraph (a replay cannot change its row count)."""
        return len(set(self._sizes)) == 1 and self._sizes[0] == self.batch_size

    @property
    def solar_vecs(self):
        """The distinct Sun_Angle rows of the table, [K, 3] numpy (`train_data["Color_Loader"].solar_vecs`): one device pass, once."""
        if self._solar_vecs is None:
            self._solar_vecs = torch.unique(self.table[:, 11:14], dim=0).cpu().numpy()
        return self._solar_vecs

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def next_into(self, buffers):
        """Draw the next batch into caller-owned tensors: `buffers` maps data_dict names (+ "Row_Index", int64 [B]) to [>= batch_size, w] float32 tensors
        on the table's device; names that are missing are not produced.  Returns the row count.  Safe inside a stream capture when `graph_safe`."""
        unknown = set(buffers) - set(FIELDS)
        if unknown:
            raise ValueError(f"DeviceRayLoader.next_into: unknown outputs {sorted(unknown)}")
        args = [None] * len(FIELDS)
        for k, t in buffers.items():
            args[FIELDS[k][0]] = t
        capturing = torch.cuda.is_current_stream_capturing()
        if capturing and not self.graph_safe:
            raise RuntimeError("DeviceRayLoader: the epoch's last batch is short - a captured draw replays with a fixed row count (use drop_last=True)")
        rows = self._sizes[self._batch]
        self._op(self._handle, self.table, *args)
        if not capturing:
            self._batch = (self._batch + 1) % self.batches_per_epoch
        return rows

    def next(self):
        """The reference's data_dict (Net_tool.get_data, mg_run_NeRF.py:229-264) of the next batch, in fresh device tensors."""
        B = self.batch_size
        flat = torch.empty(B * 28, device=self.device)
        bufs, off = {}, 0
        for k in _DICT_KEYS:
            w = FIELDS[k][1]
            bufs[k] = flat[off:off + B * w].view(B, w)
            off += B * w
        rows = self.next_into(bufs)
        out = bufs if rows == B else {k: v[:rows] for k, v in bufs.items()}
        if self.dsm_distance is not None:
            out["Dist_to_Surf_GT"], out["Dist_to_Surf_Prior"] = self.dsm_distance.get_Dist(out["Top"], out["Bot"])
        return out

    # -- position ------------------------------------------------------------------------------------------------------
    def get_state(self):
        """(epoch, batch_in_epoch, draws) read from the device (synchronises the current stream)."""
        s = np.zeros(4, dtype=np.int64)
        _lib.check(_lib.lib().snerf_loader_get_state(self._handle, s.ctypes.data, self._stream()), "snerf_loader_get_state")
        return int(s[0]), int(s[1]), int(s[2])

    def set_state(self, epoch, batch, draws):
        s = np.array([epoch, batch, draws, 0], dtype=np.int64)
        _lib.check(_lib.lib().snerf_loader_set_state(self._handle, s.ctypes.data, self._stream()), "snerf_loader_set_state")
        self._batch = int(batch)

    def state_dict(self):
        epoch, batch, draws = self.get_state()
        return {"seed": self.seed, "epoch": epoch, "batch": batch, "draws": draws}

    def load_state_dict(self, state):
        """Continue where `state` was taken: the same batches follow (the table, batch size and rank layout must be the ones of that run)."""
        if int(state["seed"]) != self.seed:
            raise ValueError(f"DeviceRayLoader.load_state_dict: the state was taken under seed {state['seed']}, this loader has seed {self.seed}")
        self.set_state(int(state["epoch"]), int(state["batch"]), int(state["draws"]))
