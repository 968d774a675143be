"""Float64 statements of the loss terms behind snerf_loss_all_forward / _backward (csrc/train_kernels.hip loss_all_*_kernel; season_nerf::loss_terms_all):
the MSE or Barron's adaptive colour loss, without or with the DSM-prior phase (Eval_Tools_2.py:361-450).  Shared by tests/test_loss_all_refs.py (CPU: the closed forms
against torch.autograd on season_nerf_amd/adaptive_loss.py, the conditions on the cases) and tests/test_gpu_loss_all.py (the kernels against float64).

Two statements:
  * `nll_closed(x, alpha, scale)` - numpy float64, closed form: the mean negative log-likelihood, its gradient with respect to x, alpha and scale.
    nll(x) = rho + log c + log Z(alpha);  z = (x / c)^2, b = |alpha - 2| + eps, d = alpha +- eps, u = 1 + z / b, p = d / 2, rho = (b / d)(u^p - 1):
        d rho / d x     = (x / c^2) u^(p-1)
        d rho / d c     = -(z / c) u^(p-1)
        d rho / d alpha = (s / d - b / d^2)(u^p - 1) + (b / d) u^p (ln u / 2 - p s z / (b^2 u)),   s = sign(alpha - 2) (0 at 2, as torch.abs differentiates)
    log Z: the cubic Hermite form on adaptive_loss._table() and its derivative.  `drop_db=True` is the mutation of the host test: s = 0
    (`drop_db="inner"`: s = 0 in the last term only, b a constant inside u).
  * `reference(h, flags, dt)` - every term, the weight vector and every gradient of a configuration as training.get_loss forms them, with torch ops on the
    CPU in dtype `dt` through adaptive_loss.py's own functions and torch.autograd, alpha and scale as leaves: float64 is the yardstick, float32 on the same
    float32 inputs measures what float32 arithmetic costs on them (E_ref).
"""
import numpy as np
import torch

from season_nerf_amd import adaptive_loss as al

EPS = al._EPS
ADAPTIVE, PRIOR, SKY_DETACHED = 1, 2, 4
CONFIGS = {"mse-free": 0, "adaptive-free": ADAPTIVE, "adaptive-prior": ADAPTIVE | PRIOR | SKY_DETACHED, "mse-prior": PRIOR | SKY_DETACHED}
NAMES = {0: ("Solar_Correction", "Solar_Correction_2", "Sky_Color_Var", "Albedo_Color", "Color"),
         1: ("Solar_Correction", "Solar_Correction_2", "Sky_Color_Var", "Albedo_Color", "Color_ada", "Color_alpha", "Color_width", "Color"),
         3: ("Solar_Correction", "Solar_Correction_2", "Sky_Color_Var", "Albedo_Color", "Alpha_Adjust_ada", "Color_ada", "Color_alpha", "Color_width",
             "Alpha_Adjust", "Alpha_alpha", "Alpha_width", "Color"),
         2: ("Solar_Correction", "Solar_Correction_2", "Sky_Color_Var", "Albedo_Color", "Color", "Alpha_Adjust")}
LOGGED = ("Solar_Correction_2", "Color_alpha", "Color_width", "Alpha_alpha", "Alpha_width")
# the alpha set of the tests (float32 values): the singular point, one ulp below it, both sides near it, the bulk of the range, near both bounds of the
# reference's loss objects.  nextafter(2, 3) and the lower bound 0.001 are left out on purpose: the float32 evaluation is itself 1-20 % off there, and a
# tolerance built on it would hide a failure.
ALPHAS = [float(np.float32(a)) for a in (2.0, np.nextafter(np.float32(2), np.float32(1)), 2.001, 1.999, 1.3, 0.2, 2.69, 2.989)]
# (D, scale, rows): the host cases
HOST_CASES = [(3, 0.03, 4099), (3, 0.0101, 4099), (1, 0.5, 5547 * 40), (1, 0.051, 300 * 96)]


def residuals(r, rows, D):
    """float32 residuals as the step forms them: colour - ground truth, both in [0, 1) (D = 3); PE - PE_Supervised, both compositing weights in [0, 0.3) (D = 1)"""
    hi = 1.0 if D == 3 else 0.3
    return (r.uniform(0, hi, (rows, D)).astype(np.float32) - r.uniform(0, hi, (rows, D)).astype(np.float32)).astype(np.float32)


def logz_closed(alpha):
    a, v, s = al._table()
    h = float(a[1] - a[0])
    u = np.clip(alpha, 0.0, float(a[-1])) / h
    i = np.clip(np.floor(u).astype(np.int64), 0, len(a) - 2)
    f = u - i
    g = 1 - f
    val = (1 + 2 * f) * g * g * v[i] + f * g * g * h * s[i] + f * f * (3 - 2 * f) * v[i + 1] + f * f * (f - 1) * h * s[i + 1]
    dval = (-6 * f * g * v[i] + g * (1 - 3 * f) * h * s[i] + 6 * f * g * v[i + 1] + (3 * f * f - 2 * f) * h * s[i + 1]) / h
    return val, np.where((alpha >= 0) & (alpha <= a[-1]), dval, 0.0)


def nll_closed(x, alpha, scale, drop_db=False):
    """x [M, D] float32, alpha / scale [D] float32 -> mean nll, d / d x [M, D], d / d alpha [D], d / d scale [D]; all in float64"""
    x, alpha, c = x.astype(np.float64), np.asarray(alpha, dtype=np.float64), np.asarray(scale, dtype=np.float64)
    M, D = x.shape
    b = np.abs(alpha - 2) + EPS
    d = np.where(alpha >= 0, alpha + EPS, alpha - EPS)
    s = np.zeros_like(alpha) if drop_db is True else np.sign(alpha - 2)
    s_in = np.zeros_like(alpha) if drop_db else s            # drop_db="inner": b treated as a constant inside u = 1 + z / b only
    p = 0.5 * d
    z = (x / c) ** 2
    t = z / b
    L = np.log1p(t)
    e = np.expm1(p * L)
    up = e + 1
    q = up / (1 + t)
    rho = (b / d) * e
    lz, dlz = logz_closed(alpha)
    value = rho.sum() / (M * D) + np.mean(np.log(c) + lz)
    d_alpha = ((s / d - b / d ** 2) * e + (b / d) * up * (0.5 * L - p * s_in * t / (b * (1 + t)))).sum(0) / (M * D) + dlz / D
    d_scale = (-(z / c) * q).sum(0) / (M * D) + 1 / (c * D)
    return value, (x / c ** 2) * q / (M * D), d_alpha, d_scale


def nll_autograd(x, alpha, scale, dt):
    """the same four quantities from adaptive_loss.py's own functions and torch.autograd in dtype dt (alpha and scale are leaves)"""
    xt = torch.tensor(x, dtype=dt, requires_grad=True)
    a = torch.tensor(np.asarray(alpha, dtype=np.float32).reshape(1, -1), dtype=dt, requires_grad=True)
    c = torch.tensor(np.asarray(scale, dtype=np.float32).reshape(1, -1), dtype=dt, requires_grad=True)
    v = torch.mean(al.general_loss(xt, a, c) + torch.log(c) + al.log_base_partition_function(a))
    v.backward()
    f = lambda t: t.detach().double().numpy()
    return float(v.detach().double()), f(xt.grad), f(a.grad).reshape(-1), f(c.grad).reshape(-1)


def make_inputs(name, R, Rs, S, alpha, scale_c=0.03, scale_a=0.5):
    """seeded float32 inputs of one call: the image rays, the sun rays, the prior's PE pair, both loss objects' alpha / scale, the three weights"""
    import zlib
    r = np.random.default_rng(zlib.crc32(name.encode()))
    u = lambda *s: r.uniform(0, 1, s).astype(np.float32)
    pe = u(R, S) * np.float32(.3)
    h = {"rgb": u(R, 3), "rgb_merged": u(R, 3), "gt": u(R, 3), "albedo": u(R, 3) * np.float32(.8) + np.float32(.05), "sky": u(R, 3), "sv": u(Rs, S), "pv": u(Rs, S),
         "pe_sun": u(Rs, S) * np.float32(.1), "pe": pe, "pe_sup": (pe + (u(R, S) - np.float32(.5)) * np.float32(.2)).astype(np.float32),
         "alpha_c": np.float32([alpha, alpha, alpha]), "scale_c": np.float32([scale_c, scale_c * 1.3, scale_c * 0.8]),
         "alpha_a": np.float32([alpha]), "scale_a": np.float32([scale_a]), "w": (0.03, 1.0, 1.0)}
    return h


DIFF_INPUTS = ("rgb", "rgb_merged", "albedo", "sky", "sv", "pe", "alpha_c", "scale_c", "alpha_a", "scale_a")


def reference(h, flags, dt, g=None):
    """-> vals [n], weights [n], scale [n] (float64: the sum of the absolute parts of each value), grads {input: array or None} of sum_i g_i vals_i, all as
    float64 arrays evaluated in dtype dt"""
    ada, prior, sky_det = bool(flags & ADAPTIVE), bool(flags & PRIOR), bool(flags & SKY_DETACHED)
    names = NAMES[flags & 3]
    T = {k: torch.tensor(np.asarray(h[k]).reshape(1, -1) if k.startswith(("alpha_", "scale_")) else h[k], dtype=dt, requires_grad=k in DIFF_INPUTS)
         for k in h if k != "w"}
    w_sc, w_col, w_al = h["w"]
    R, Rs = T["rgb"].shape[0], T["sv"].shape[0]
    sq = lambda x: x * x
    mse = lambda a, b: torch.mean(sq(a - b))
    V, W, SC = {}, {}, {}
    V["Solar_Correction"] = torch.mean(torch.sum(sq(T["sv"] - T["pv"]), 1))
    absorbed = torch.sum(T["pe_sun"] * T["pv"] * T["sv"], 1)
    V["Solar_Correction_2"] = torch.mean(1 - absorbed)
    SC["Solar_Correction_2"] = 1 + float(absorbed.detach().double().abs().mean())
    x = (T["sky"] - .5) / .5
    V["Sky_Color_Var"] = torch.sum(torch.where(x > 0, sq(x), torch.zeros_like(x))) / x.numel()
    amin = torch.min(T["albedo"], 0).values
    V["Albedo_Color"] = torch.sum(torch.where(amin < .2, sq(1. - amin / .2), torch.zeros_like(amin))) / R
    for k in ("Solar_Correction", "Sky_Color_Var", "Albedo_Color"):
        W[k] = w_sc
    W["Solar_Correction_2"] = w_sc
    col = T["rgb_merged"] if h.get("use_merged", prior) else T["rgb"]
    V["Color"], W["Color"] = mse(col, T["gt"]), w_col
    if prior:
        V["Alpha_Adjust"], W["Alpha_Adjust"] = mse(T["pe"], T["pe_sup"]), w_al
    if ada:
        nll = lambda x_, a_, c_: al.general_loss(x_, a_, c_) + torch.log(c_) + al.log_base_partition_function(a_)
        part = lambda x_, a_, c_: float((al.general_loss(x_, a_, c_).mean() + torch.log(c_).abs().mean() + al.log_base_partition_function(a_).abs().mean()).detach().double())
        V["Color_ada"], W["Color_ada"] = torch.mean(nll(T["rgb"] - T["gt"], T["alpha_c"], T["scale_c"])), w_col
        SC["Color_ada"] = part(T["rgb"] - T["gt"], T["alpha_c"], T["scale_c"])
        V["Color_alpha"], V["Color_width"] = torch.mean(T["alpha_c"].detach()), torch.mean(T["scale_c"].detach())
        W["Color_alpha"] = W["Color_width"] = 1.0
        width2 = torch.mean(T["scale_c"].detach()) ** 2
        W["Solar_Correction"] = W["Solar_Correction_2"] = w_sc / width2
        if prior:
            xa = (T["pe"] - T["pe_sup"]).reshape(-1, 1)
            V["Alpha_Adjust_ada"], W["Alpha_Adjust_ada"] = torch.mean(nll(xa, T["alpha_a"], T["scale_a"])), w_al
            SC["Alpha_Adjust_ada"] = part(xa, T["alpha_a"], T["scale_a"])
            V["Alpha_alpha"], V["Alpha_width"] = torch.mean(T["alpha_a"].detach()), torch.mean(T["scale_a"].detach())
            W["Alpha_alpha"] = W["Alpha_width"] = 1.0
    f = lambda t: t.detach().double().numpy()
    vals = np.array([float(f(V[k])) for k in names])
    wts = np.array([float(f(W[k])) if torch.is_tensor(W[k]) else float(np.float32(W[k]) if dt == torch.float32 else W[k]) for k in names])
    scale = np.array([SC.get(k, abs(float(f(V[k])))) for k in names])
    grads = None
    if g is not None:
        value_only = lambda k: k in LOGGED or (k == "Sky_Color_Var" and sky_det) or (k == "Color" and ada)
        total = sum(float(gi) * V[k] for gi, k in zip(g, names) if not value_only(k))
        total.backward()
        grads = {k: (f(T[k].grad) if T[k].grad is not None else None) for k in DIFF_INPUTS}
    return vals, wts, scale, grads
