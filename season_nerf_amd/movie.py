"""The frames of the reference's fly-through films (T_NeRF_Eval_Utils/mg_movie_maker.py): a slab of parallel rays rotated by pitch and yaw about a
centre, the whole network on every sample, and a compositing with the learned solar visibility applied per sample,

    Out_Img[r] = sum_s PS_s (vis_s + (1 - vis_s) sky) col_s        HM[r] = sum_s PS_s linspace(0, 2, S)[s].

`frame_walk` renders a frame inside the field kernel (`season_nerf::frame_walk`, csrc/mlp_device.h RayFrame): sixteen floats per ray come back, no
per-sample array is formed, and the seasons shown in a frame come from one pass of the network, since only the class vector depends on the time.
`get_Img` keeps the reference's constructor and method signatures; `capture_frame`, `capture_frame_advanced` and `eval_rays_advanced` go through the walk,
`eval_rays` returns the per-sample PS and therefore uses the per-sample kernels.  The spline `script` class, `film_movie`'s path integration and
`edit_film` are host scipy / plotting and are not mirrored.
"""
import numpy as np
import torch

from .evaluator import sample_parameters_on
from .render import _f32, _ray_samples, _walks, encode_time

MAX_FRAME_TIMES = 4      # seasons per launch (include/season_nerf_hip.h SNERF_MAX_FRAME_TIMES)
_CUBE = np.array([[-1, 1.], [-1, 1], [-1, 1]])


# ------------------------------------------------------------------------------------------------ geometry
def _rotation(phi_deg, theta_deg):
    """yaw(theta) @ pitch(phi), float64 (mg_movie_maker.py:54-61)."""
    p, y = phi_deg * np.pi / 180, theta_deg * np.pi / 180
    pitch = np.array([[np.cos(p), 0, np.sin(p)], [0, 1, 0], [-np.sin(p), 0, np.cos(p)]])
    yaw = np.array([[np.cos(y), -np.sin(y), 0], [np.sin(y), np.cos(y), 0], [0, 0, 1]])
    return yaw @ pitch


def _slab(Img_Center, Img_length, phi_deg, theta_deg, Img_Size, zs):
    """The lattice points with the heights `zs` (before the rotation) -> [Img_Size[0], Img_Size[1], len(zs), 3] float64: row i at y = linspace(-l0, l0)[i],
    column j at x = linspace(-l1, l1)[j], rotated and moved to the centre with the reference's operations (a batched 3x3 @ 3x1 product, then the sum)."""
    xs, ys = np.linspace(-Img_length[1], Img_length[1], Img_Size[1]), np.linspace(-Img_length[0], Img_length[0], Img_Size[0])
    grid = np.stack(np.meshgrid(xs, ys, np.asarray(zs, dtype=np.float64)), -1)[..., None]
    pts = _rotation(phi_deg, theta_deg).reshape(1, 1, 1, 3, 3) @ grid + np.asarray(Img_Center, dtype=np.float64).reshape(1, 1, 1, 3, 1)
    return pts[..., 0]


def sample_rays_projective(Img_Center, Img_length, phi_deg, theta_deg, Img_Size):
    """mg_movie_maker.py:52-70 -> Rays [Img_Size[0], Img_Size[1], Img_Size[2], 3] float64 (sample k of a ray at height linspace(l2, -l2)[k] before the
    rotation) and delta, the distance between the first two samples of ray (0, 0): the spacing of every ray's samples."""
    rays = _slab(Img_Center, Img_length, phi_deg, theta_deg, Img_Size, np.linspace(Img_length[2], -Img_length[2], Img_Size[2]))
    return rays, np.sqrt(np.sum((rays[0, 0, 1] - rays[0, 0, 0]) ** 2, -1))


def frame_end_planes(Img_Center, Img_length, phi_deg, theta_deg, Img_Size):
    """Only what the walk needs of `sample_rays_projective`: the top and bottom planes [H,W,3] as float32 (the float64 lattice, cast) and delta (float64).
    [H,W,S,3] is never formed: two planes, and the first two samples of one ray for delta."""
    zs = np.linspace(Img_length[2], -Img_length[2], Img_Size[2])
    ends = _slab(Img_Center, Img_length, phi_deg, theta_deg, Img_Size, zs[[0, -1]])
    first = _slab(Img_Center, Img_length, phi_deg, theta_deg, (1, 1), zs[:2])      # linspace(-l, l, 1) = [-l]: ray (0, 0) whatever the image size
    delta = np.sqrt(np.sum((first[0, 0, 1] - first[0, 0, 0]) ** 2, -1))
    return ends[:, :, 0].astype(np.float32), ends[:, :, 1].astype(np.float32), delta


# ------------------------------------------------------------------------------------------------ the walk
class FrameWalk:
    """What `frame_walk` returns.  `rows`: a list of [R,16] tensors, one per launch of up to MAX_FRAME_TIMES seasons (include/season_nerf_hip.h
    snerf_field_frame_walk: season k of a launch at [3k .. 3k+2], [12] sum PS, [13] sum PS s, [14] the optical depth walked, [15] sum PS vis);
    slots 12..15 are read from the first launch.  Everything derived is float64 on the rows' device."""

    def __init__(self, rows, n_times, n_samples):
        self.rows = [rows] if torch.is_tensor(rows) else list(rows)
        self.n_times, self.n_samples = int(n_times), int(n_samples)
        if not self.rows or not (len(self.rows) - 1) * MAX_FRAME_TIMES < self.n_times <= len(self.rows) * MAX_FRAME_TIMES:
            raise ValueError(f"FrameWalk: {len(self.rows)} launches of up to {MAX_FRAME_TIMES} seasons do not hold {self.n_times} seasons")

    @property
    def n_rays(self):
        return self.rows[0].shape[0]

    @property
    def rgb(self):
        """[T,R,3] float64."""
        per = [r[:, :3 * MAX_FRAME_TIMES].double().reshape(-1, MAX_FRAME_TIMES, 3).permute(1, 0, 2) for r in self.rows]
        return torch.cat(per, 0)[:self.n_times]

    def images(self, shape):
        """Out_Img of every season (mg_movie_maker.py:153-161) -> [T,H,W,3]."""
        return self.rgb.reshape(self.n_times, int(shape[0]), int(shape[1]), 3)

    def height_map(self, shape):
        """HM = sum_s PS_s linspace(0, 2, S)[s] (mg_movie_maker.py:185-186) -> [H,W]."""
        return (2.0 * self.rows[0][:, 13].double() / (self.n_samples - 1)).reshape(int(shape[0]), int(shape[1]))

    @property
    def opacity(self):
        """sum_s PS_s -> [R]."""
        return self.rows[0][:, 12].double()

    @property
    def transmittance(self):
        """exp(-optical depth walked): what is left of the ray behind its last walked sample -> [R]."""
        return torch.exp(-self.rows[0][:, 14].double())


def frame_rows(rho, col_raw, vis, adjust, sky, class_vecs, delta):
    """The sixteen numbers per ray of one launch from per-sample arrays, in the arrays' dtype: rho [R,S], col_raw [R,S,3], vis [R,S], adjust [R,S,C,3],
    sky [3], class_vecs [T,C] with T <= MAX_FRAME_TIMES, delta [R,S] (0 where a sample does not count) -> [R,16].  PV is the exclusive prefix."""
    y = rho * delta
    c = torch.cumsum(torch.cat([torch.zeros_like(y[:, :1]), y], 1), 1)
    ps = torch.exp(-c[:, :-1]) * (1.0 - torch.exp(-y))
    shade = vis.unsqueeze(-1) + (1.0 - vis.unsqueeze(-1)) * sky.reshape(1, 1, 3)
    out = torch.zeros(rho.shape[0], 16, dtype=rho.dtype, device=rho.device)
    for k in range(class_vecs.shape[0]):
        col = torch.sigmoid(col_raw + torch.einsum("rscj,c->rsj", adjust, class_vecs[k]))
        out[:, 3 * k:3 * k + 3] = (ps.unsqueeze(-1) * shade * col).sum(1)
    idx = torch.arange(rho.shape[1], device=rho.device, dtype=rho.dtype)
    out[:, 12], out[:, 13], out[:, 14], out[:, 15] = ps.sum(1), (ps * idx).sum(1), c[:, -1], (ps * vis).sum(1)
    return out


def _outside(p, valid_range):
    """Rays_Reshape_bad of eval_rays (mg_movie_maker.py:141-143): strictly outside the range on any axis."""
    lo = torch.tensor(np.asarray(valid_range, dtype=np.float64)[:, 0], device=p.device)
    hi = torch.tensor(np.asarray(valid_range, dtype=np.float64)[:, 1], device=p.device)
    return ((p.double() < lo) | (p.double() > hi)).any(-1)


def _frame_layerwise(net, top, bot, tv, S, delta, sun, tim, class_vecs, valid_range):
    """The rows of `frame_walk` for a chunk of rays from `forward_seperate` on the sample points and float64 sums: networks the frame-walk kernels do
    not serve, and a valid range other than the cube.  -> list of [n,16] float64, one per MAX_FRAME_TIMES seasons."""
    n = top.shape[0]
    p, _ = _ray_samples(top, bot, tv, S, False)          # the points only: a frame's delta is the caller's `delta`, not the ray's length / S
    rho, col_raw, vis, sky, _, adj = net.forward_seperate(p.reshape(-1, 3), sun.reshape(1, 3).expand(n * S, 3), tim.reshape(1, 4).expand(n * S, 4))
    d = torch.full((n, S), float(delta), dtype=torch.float64, device=top.device)
    d = torch.where(_outside(p, valid_range), torch.zeros_like(d), d)
    f = lambda a, *s: a.detach().double().reshape(n, S, *s)
    cv = class_vecs.double()
    return [frame_rows(f(rho), f(col_raw, 3), f(vis), f(adj, net.n_classes, 3), sky[0].detach().double(), cv[k:k + MAX_FRAME_TIMES], d)
            for k in range(0, cv.shape[0], MAX_FRAME_TIMES)]


def frame_walk(net, top, bot, S, delta, sun, times=None, class_vecs=None, *, early_out=True, valid_range=None):
    """A film frame's rays top -> bot ([R,3], or planes [H,W,3]) with S >= 2 end-point-inclusive samples of spacing `delta`, one sun direction `sun` [3]
    (passed to the network as given) and the seasons `times` (fractions of a year) or `class_vecs` [T,C] -> `FrameWalk`.

    On a fused bf16x3 model (widths 64 / 256 / 512) in eval mode one launch of `season_nerf::frame_walk` per MAX_FRAME_TIMES seasons and chunk of rays:
    the whole network with the shading and the transmittance scan in the kernel, 64 bytes out per ray.  The sky colour and the class vectors come from
    the group network.  early_out: a workgroup whose rays have all passed optical depth 18 skips their remaining samples.  A sample outside
    `valid_range` (None = the cube [-1,1]^3) does not count, as in the reference.  Anything else - int8-resolved models, the one-term mode, a width without a
    fused kernel, a module in training mode, a valid range other than the cube - gets the same sixteen numbers in float64 from `forward_seperate` on the
    sample points: slower, and correct."""
    with torch.no_grad():
        dev = top.device
        top, bot = top.float().reshape(-1, 3).contiguous(), bot.float().reshape(-1, 3).contiguous()
        R, S, delta = top.shape[0], int(S), float(delta)
        if bot.shape != top.shape:
            raise ValueError(f"frame_walk: top {tuple(top.shape)} and bot {tuple(bot.shape)} must hold the same rays")
        if S < 2 or not (np.isfinite(delta) and delta > 0):
            raise ValueError(f"frame_walk: needs S >= 2 and a finite positive delta, got S = {S}, delta = {delta}")
        if (times is None) == (class_vecs is None):
            raise ValueError("frame_walk: give either times or class_vecs")
        sun = _f32(np.asarray(sun.detach().cpu() if torch.is_tensor(sun) else sun, dtype=np.float64).reshape(3), dev)
        if times is not None:
            tims = _f32(np.stack([encode_time(float(a)) for a in np.asarray(times, dtype=np.float64).reshape(-1)]), dev)
            class_vecs = net.get_class_only(tims)
        else:
            tims = _f32(encode_time(0.0).reshape(1, 4), dev)
        class_vecs = class_vecs.detach().float().reshape(-1, net.n_classes).contiguous()
        T = class_vecs.shape[0]
        if T < 1:
            raise ValueError("frame_walk: needs at least one season")
        cube = valid_range is None or np.array_equal(np.asarray(valid_range, dtype=np.float64), _CUBE)
        tv = sample_parameters_on(dev, S, eval_mode=True, include_end_pt=True)
        n_launch = (T + MAX_FRAME_TIMES - 1) // MAX_FRAME_TIMES
        if _walks(net) and not net.training and cube:
            from .network import _ops
            sky = net._groups(tims[:1], sun.reshape(1, 3))[2][0].contiguous()
            flags = 2 | (0 if early_out else 4)
            rows = [torch.empty(R, 16, device=dev) for _ in range(n_launch)]
            chunk = 1 << 22
            for k in range(n_launch):
                cv = class_vecs[k * MAX_FRAME_TIMES:(k + 1) * MAX_FRAME_TIMES].contiguous()
                for i in range(0, R, chunk):
                    j = min(R, i + chunk)
                    rows[k][i:j] = _ops().frame_walk(net.device_model(), top[i:j], bot[i:j], tv, delta, sun, sky, cv, flags)
        else:
            rows = [torch.empty(R, 16, device=dev, dtype=torch.float64) for _ in range(n_launch)]
            # sized as ray_surface sizes the layer-wise engine's chunks: ~32 [points x width] fp32 arrays, ~12 GB of workspace
            chunk = min(1 << 16, max(64, int(12e9 / (128.0 * net.layer_width)) // S))
            for i in range(0, R, chunk):
                j = min(R, i + chunk)
                part = _frame_layerwise(net, top[i:j], bot[i:j], tv, S, delta, sun, tims[0], class_vecs, _CUBE if cube else valid_range)
                for k in range(n_launch):
                    rows[k][i:j] = part[k]
        return FrameWalk(rows, T, S)


# ------------------------------------------------------------------------------------------------ the reference's call boundary
class get_Img():
    """mg_movie_maker.py:72-187 under the reference's names.  `max_batch_size` and `per_img_tqdm` are accepted and not needed: a frame is one launch."""

    def __init__(self, network, device, valid_range=np.array([[-1, 1.], [-1, 1], [-1, 1]]), max_batch_size=100, per_img_tqdm=True):
        self.network = network
        self.valid_range = valid_range
        self.device = device
        self.max_batch_size = max_batch_size
        self.per_img_tqdm = per_img_tqdm

    def _walk(self, top, bot, S, delta, Solar_Angle, times):
        dev = torch.device(self.device)
        return frame_walk(self.network, _f32(top, dev), _f32(bot, dev), S, delta, Solar_Angle, times=times, valid_range=self.valid_range)

    def capture_frame(self, Img_Center, Img_length, phi_deg, theta_deg, Img_Size, Solar_Angle, Time, use_Time=True, Sky_Color=None):
        """-> Img [H,W,3] float64 numpy."""
        top, bot, delta = frame_end_planes(Img_Center, Img_length, phi_deg, theta_deg, Img_Size)
        fw = self._walk(top, bot, Img_Size[2], delta, Solar_Angle, [Time])
        return fw.images(top.shape[:2])[0].cpu().numpy()

    def capture_frame_advanced(self, Img_Center, Img_length, phi_deg, theta_deg, Img_Size, Solar_Angle, Time, use_Time=True, Sky_Color=None):
        """-> (Imgs: one [H,W,3] per entry of Time, HM [H,W]); the reference's third result, a plot of the camera angle, is reporting and left out."""
        top, bot, delta = frame_end_planes(Img_Center, Img_length, phi_deg, theta_deg, Img_Size)
        fw = self._walk(top, bot, Img_Size[2], delta, Solar_Angle, np.asarray(Time, dtype=np.float64).reshape(-1))
        return list(fw.images(top.shape[:2]).cpu().numpy()), fw.height_map(top.shape[:2]).cpu().numpy()

    def eval_rays(self, Rays, Solar_Angle, Time, use_Time=True, Sky_Color=None, delta=None):
        """-> (Out_Img [H,W,3], PS [H,W,S,1]), float64 numpy: the per-sample kernels (`T_NeRF.forward` on the float32 points) and float64 sums."""
        if delta is None:
            raise ValueError("get_Img.eval_rays: delta is required, as in the reference")
        with torch.no_grad():
            dev = torch.device(self.device)
            Rays = np.asarray(Rays)
            H, W, S = Rays.shape[:3]
            p = _f32(Rays.reshape(-1, 3), dev)
            n = p.shape[0]
            sun = _f32(np.asarray(Solar_Angle, dtype=np.float64).reshape(1, 3), dev).expand(n, 3)
            tim = _f32(encode_time(float(Time)).reshape(1, 4), dev).expand(n, 4)
            rho, col, vis, sky, _, _ = self.network(p, sun, tim)
            y = torch.where(_outside(p, self.valid_range), torch.zeros(n, dtype=torch.float64, device=dev), rho.detach().double().reshape(n)).reshape(H * W, S) * float(delta)
            c = torch.cumsum(torch.cat([torch.zeros_like(y[:, :1]), y], 1), 1)
            ps = torch.exp(-c[:, :-1]) * (1.0 - torch.exp(-y))
            vis = vis.detach().double().reshape(H * W, S, 1)
            final = (vis + (1.0 - vis) * sky[0].detach().double().reshape(1, 1, 3)) * col.detach().double().reshape(H * W, S, 3)
            img = (ps.unsqueeze(-1) * final).sum(1)
            return img.reshape(H, W, 3).cpu().numpy(), ps.reshape(H, W, S, 1).cpu().numpy()

    def eval_rays_advanced(self, Rays, Solar_Angle, Time, use_Time=True, Sky_Color=None, delta=None):
        """-> (Out_Imgs: one [H,W,3] per entry of Time, HM [H,W]) from the rays' end planes Rays[:, :, 0] and Rays[:, :, -1] through the walk."""
        if delta is None:
            raise ValueError("get_Img.eval_rays_advanced: delta is required, as in the reference")
        Rays = np.asarray(Rays)
        H, W, S = Rays.shape[:3]
        fw = self._walk(Rays[:, :, 0].astype(np.float32), Rays[:, :, -1].astype(np.float32), S, delta, Solar_Angle, np.asarray(Time, dtype=np.float64).reshape(-1))
        return list(fw.images((H, W)).cpu().numpy()), fw.height_map((H, W)).cpu().numpy()
