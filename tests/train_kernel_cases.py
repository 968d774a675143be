"""Cases and float64 references for the element kernels of the training engine (csrc/train_kernels.hip), run one launcher at a time
through snerf_train_kernel_debug.  Shared by tests/test_gpu_train_kernels.py (the kernels against these references on the GPU) and
tests/test_train_kernel_refs.py (the references against torch.autograd / the oracle, and the conditions that keep the cases honest, on the CPU).

A case is data only: the operation, its sizes and scalars, one buffer description per pointer slot and the name of its reference formula.  A
reference takes the case's fp32 inputs converted to a dtype `dt` and evaluates the operation's formula in that dtype: float64 is the yardstick,
float32 the measure of what fp32 arithmetic costs on these very inputs (E_ref).  Two things stay as the kernels define them in either dtype,
because they are part of the operation and not of its rounding: the encodings' argument 2^j * fl32(fl32(pi/2) * x) (and the fp32 lerp of the ray
form), and the double-precision moments of the shifted BatchNorm sums up to the point where the kernel converts them to fp32.

Every reference returns {buffer name: Out}.  Out.kind is "sum" (a reduction over the rows: `scale` is the float64 sum of the absolute terms per
column, `first` / `last` the contribution of the first / last row, so that value - first, value - last and value + last are the reference with a
row left out or counted twice) or "elem" (scale: the output's magnitude, or 1 for outputs in [-1, 1]).

Tolerance (the issue's rule, as tests/test_gpu_compositing.py measures its own): a kernel value lies within FACTOR * (E_ref + 2^-24 * scale) of
float64, E_ref = the largest deviation of the fp32 evaluation from float64 over that output of that case.  One group of outputs has a wider margin,
with its reason: CHAIN_FACTOR below.
"""
import zlib
from collections import namedtuple

import numpy as np

FACTOR = 4.0
EPS = 2.0 ** -24
SENTINEL = np.float32(-7.25e33)
# The one margin above FACTOR: the column sums of the SineLayer column passes (colreduce out0 / out1, bn_bwd2 dbias; scalar and vector kernels, every
# case alike).  A block adds its rows in sequential fp32 chains - a thread walks down its rows, then one thread adds the row phases from LDS one after the
# other: 256 additions in a row at C = 4 (one thread per row, 256 row phases) - where the fp32 reference adds pairwise (a tree of depth 8 for 256 terms).
# A chain of n additions of terms of one size collects n rounding errors of up to half an ulp of the growing partial sum: its deviation from the float64
# sum grows like sqrt(n) ulp of the sum of the absolute terms against sqrt(log2 n) for the tree.  Emulated on the CPU from float64 quantities (the float64
# terms of colreduce-m1-C4-M256 and colreduce-m2-C4-M256 rounded to fp32 and added in the kernel's order): 0.93 and 0.86 of the FACTOR = 4 tolerance
# - at the edge, where a correct kernel with one more rounding per term can land on either side.  The margin is sqrt(256) = 16 ulp-sums instead of 4;
# the conditions of tests/test_train_kernel_refs.py (a row left out misses by 10x) are asserted against this wider tolerance.
CHAIN_FACTOR = 16.0

KERNELS = {"pe_points_kernel": 0, "pe_small_kernel": 1, "colreduce_kernel": 2, "colpass_vec_kernel<1>": 3, "colpass_vec_kernel<2>": 4,
           "colpass_vec_kernel<3>": 5, "colpass_vec_kernel<4>": 6, "bn_bwd2_kernel": 7, "bn_finalize_kernel": 8, "bn_finalize_shifted_kernel": 9,
           "act_sums_finalize_kernel": 10, "act_table_kernel": 11, "sin_fwd_kernel": 12, "sin_fwd_vec_kernel": 13, "thin_dgrad_kernel<false>": 14,
           "thin_dgrad_kernel<true>": 15, "point_out_fwd_kernel": 16, "point_out_bwd_kernel": 17, "softmax_kernel": 18, "softmax_bwd_kernel": 19,
           "sigmoid_kernel": 20, "sigmoid_bwd_kernel": 21, "colsum_kernel": 22, "copy_cols_kernel": 23, "bcast_rows_kernel": 24,
           "reduce_rows_kernel": 25, "fill_zero_kernel": 26, "copy_f32_kernel": 27, "fill_zero_bytes_kernel": 28, "copy_bytes_kernel": 29}

Out = namedtuple("Out", "value scale kind first last factor", defaults=(None, None, FACTOR))
# a pointer slot: data = the logical fp32 (or float64) array, [M, C] or 1-D; ld = its row stride in the device buffer (1-D: None); role "in" (padding
# NaN), "out" (everything a sentinel before the call) or "inout" (data, padding a sentinel); off = elements the base is moved off its 256-byte alignment
Buf = namedtuple("Buf", "name data ld role off", defaults=(0,))
Case = namedtuple("Case", "id op sizes scalars bufs ref kernel par")


def tolerance(e_ref, scale, factor=FACTOR):
    return factor * (e_ref + EPS * scale)


def rng_for(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------------------------------ references
def _sum_out(terms, init, alpha=1.0, factor=FACTOR):
    """out = init + alpha * sum over rows of terms [M, C] (terms in the evaluation's dtype)"""
    dt = terms.dtype
    a = dt.type(alpha)
    v = init.astype(dt) + a * np.sum(np.ascontiguousarray(terms.T), axis=1, dtype=dt)      # (contiguous axis: numpy adds pairwise, as a tree of partial sums)
    scale = np.abs(init.astype(np.float64)) + abs(float(alpha)) * np.sum(np.abs(terms.astype(np.float64)), axis=0)
    return Out(v, scale, "sum", a * terms[0], a * terms[-1], factor)


def _elem(v, unit=False):
    return Out(v, np.ones(v.shape) if unit else np.abs(v.astype(np.float64)), "elem")


def ref_colreduce(v, par, dt):
    z = v["Z"]
    if par["mode"] == 0:
        d = z - v["mu"]
        return {"out0": _sum_out(d * d, v["out0"], factor=CHAIN_FACTOR)}
    if par["mode"] == 1:
        xh = (z - v["mu"]) * v["istd"]
        dy = v["D"] * np.cos(v["gamma"] * xh + v["beta"])
        return {"out0": _sum_out(dy, v["out0"], factor=CHAIN_FACTOR), "out1": _sum_out(dy * xh, v["out1"], factor=CHAIN_FACTOR), "D": _elem(v["D"])}
    dz = v["D"] * np.cos(z)
    return {"D": _elem(dz), "out0": _sum_out(dz, v["out0"], par["alpha"], CHAIN_FACTOR)}


def ref_bn_bwd2(v, par, dt):
    xh = (v["Z"] - v["mu"]) * v["istd"]
    dy = v["D"] if par["d_is_dy"] else v["D"] * np.cos(v["gamma"] * xh + v["beta"])
    mg = dt.type(par["M_global"])
    dz = (v["gamma"] * v["istd"]) * (dy - v["sdy"] / mg - xh * (v["sdyx"] / mg))
    return {"D": _elem(dz), "dbias": _sum_out(dz, v["dbias"], par["alpha"], CHAIN_FACTOR)}


def ref_sin_fwd(v, par, dt):
    z = v["Z"]
    if par["bn"]:
        z = v["gamma"] * ((z - v["mu"]) * v["istd"]) + v["beta"]
    return {"H": _elem(np.sin(z), unit=True)}


def ref_bn_finalize(v, par, dt):
    M = dt.type(par["M"])
    if par["stage"] == 0:
        return {"mean": _elem(v["colsum"] / M)}
    if par["stage"] == 2:
        return {"istd": _elem(1 / np.sqrt(v["m2"] + dt.type(1e-5)))}
    var_b = v["m2"] / M
    var_u = v["m2"] / dt.type(par["M"] - 1) if par["M"] > 1 else var_b
    return {"istd": _elem(1 / np.sqrt(var_b + dt.type(1e-5))),
            "running_mean": _elem(dt.type(0.99) * v["running_mean"] + dt.type(0.01) * v["mean"]),
            "running_var": _elem(dt.type(0.99) * v["running_var"] + dt.type(0.01) * var_u)}


def ref_bn_finalize_shifted(v, par, dt):
    C, M = par["C"], par["M"]
    st = v["stats"].astype(np.float64)                       # the moments stay double in either evaluation (module docstring)
    m1, m2 = st[:C] / M, st[C:] / M
    shift = np.float32(par["alpha"]) * v["bias"].astype(np.float32)          # the kernel's fp32 product, part of the operation
    mu = shift.astype(np.float64) + m1
    var_b = np.maximum(m2 - m1 * m1, 0.0)
    var_u = var_b * M / (M - 1) if M > 1 else var_b
    mean = mu.astype(dt)
    istd = 1 / np.sqrt(var_b.astype(dt) + dt.type(1e-5))
    out = {"mean": _elem(mean), "istd": _elem(istd),
           "running_mean": _elem(dt.type(0.99) * v["running_mean"] + dt.type(0.01) * mean),
           "running_var": _elem(dt.type(0.99) * v["running_var"] + dt.type(0.01) * var_u.astype(dt)),
           "stats": Out(np.zeros(2 * C, dtype=dt), np.zeros(2 * C), "elem")}
    if par["tab"]:
        out["tab"] = _elem(ref_act_table({"mu": mean, "istd": istd, "gamma": v["gamma"], "beta": v["beta"]}, {"bn": True}, dt)["dst"].value)
    return out


def ref_act_sums_finalize(v, par, dt):
    C = par["C"]
    st = v["stats"].astype(dt)
    s0, s1 = dt.type(par["scale0"]) * st[:C], st[C:]
    out = {"out0": _elem(s0), "out1": _elem(s1), "stats": Out(np.zeros(2 * C, dtype=dt), np.zeros(2 * C), "elem")}
    if "acc0" in v:
        out.update(acc0=_elem(v["acc0"] + s0), acc1=_elem(v["acc1"] + s1))
    return {k: o for k, o in out.items() if k in v}


def ref_act_table(v, par, dt):
    inv2pi = dt.type(1 / (2 * np.pi))
    if not par["bn"]:
        n = par["n"]
        return {"dst": _elem(np.concatenate([np.full(n, inv2pi, dtype=dt), np.zeros(n, dtype=dt)]))}
    a = v["gamma"] * v["istd"]
    return {"dst": _elem(np.concatenate([a * inv2pi, (v["beta"] - a * v["mu"]) * inv2pi]))}


def ref_thin_dgrad(v, par, dt):
    K, N = par["K"], par["N"]
    W = v["W"][:K].copy()
    if par["w3"]:
        W[3] = v["W3"][0]
    c = dt.type(par["alpha"]) * (v["D"][:, :K] @ W)
    if par["accumulate"]:
        c = c + v["C"]
    if not par["act"]:
        return {"C": _elem(c)}
    tab = v["etab"]
    c = c * np.cos(dt.type(2 * np.pi) * (tab[:N] * v["ez"] + tab[N:]))
    xh = (v["ez"] - v["emu"]) * v["eistd"] if par["bn"] else np.zeros_like(c)
    st = v["stats"].astype(dt)
    s0, s1 = _sum_out(c, st[:N]), _sum_out(c * xh, st[N:])
    cat = lambda a, b: None if a is None else np.concatenate([a, b])
    return {"C": _elem(c), "stats": Out(cat(s0.value, s1.value), cat(s0.scale, s1.scale), "sum", cat(s0.first, s1.first), cat(s0.last, s1.last))}


def _sigmoid(x):
    return 1 / (1 + np.exp(-x))


def ref_point_out_fwd(v, par, dt):
    out = {}
    S, C = par["n_samples"], par["C"]
    if "rho" in v:
        raw = v["head"][:, 3]
        with np.errstate(over="ignore"):
            out["rho"] = _elem(np.where(raw > 20, raw, np.log1p(np.exp(np.minimum(raw, 30)))))
    if "sv" in v:
        out["sv"] = _elem(_sigmoid(v["sv_raw"]), unit=True)
    if "col" in v:
        n = v["head"].shape[0]
        p = v["cls"][np.arange(n) // S]                              # [n, C]
        ac = np.einsum("ick,ic->ik", v["adj"].reshape(n, C, 3), p)
        out["col"] = _elem(_sigmoid(v["head"][:, :3] + ac), unit=True)
        if "adjust_col" in v:
            out["adjust_col"] = _elem(ac)
    return out


def ref_point_out_bwd(v, par, dt):
    out = {}
    S, C = par["n_samples"], par["C"]
    if "d_head" in v:
        n = v["head"].shape[0]
        raw = v["head"][:, 3]
        d_head = np.zeros((n, 4), dtype=dt)
        if "d_rho" in v:
            d_head[:, 3] = v["d_rho"] * np.where(raw > 20, dt.type(1), _sigmoid(raw))
        dpre = np.zeros((n, 3), dtype=dt)
        if "d_col" in v:
            y = v["col"]
            dpre = v["d_col"] * y * (1 - y)
        d_head[:, :3] = dpre
        out["d_head"] = _elem(d_head)
        p = v["cls"][np.arange(n) // S]
        if "d_adj" in v:
            out["d_adj"] = _elem((p[:, :, None] * dpre[:, None, :]).reshape(n, 3 * C))
        if "d_cls" in v:
            terms = np.einsum("ik,ick->ic", dpre, v["adj"].reshape(n, C, 3))      # one term per point and class
            R = v["d_cls"].shape[0]
            val = v["d_cls"].astype(dt).copy()
            scale = np.abs(v["d_cls"].astype(np.float64))
            first, last = np.zeros((R, C), dtype=dt), np.zeros((R, C), dtype=dt)
            for g in range(R):
                t = terms[g * S:(g + 1) * S]
                val[g] += np.sum(t, axis=0, dtype=dt)
                scale[g] += np.sum(np.abs(t.astype(np.float64)), axis=0)
                first[g], last[g] = t[0], t[-1]                  # per ray: its first and its last sample
            out["d_cls"] = Out(val, scale, "sum", first, last)
    if "d_sv_raw" in v:
        y = v["sv"]
        out["d_sv_raw"] = _elem(v["d_sv"] * y * (1 - y))
    return out


HALF_PI32 = np.float32(1.57079637050628662109375)


def pe_argument(x32, j):
    """2^j * fl32(fl32(pi/2) * x): the fp32 product is exact in float64, so one conversion rounds it as the kernels' __fmul_rn does"""
    a0 = (x32.astype(np.float64) * np.float64(HALF_PI32)).astype(np.float32)
    return a0 * np.float32(2.0 ** j)


def pe_features(x32, n_freq, dt):
    """[rows, D] -> [rows, D * (2 n_freq + 1)]: x, then per dimension cos of the n_freq arguments, then their sines"""
    rows, D = x32.shape
    cols = [x32.astype(dt)]
    for d in range(D):
        args = np.stack([pe_argument(x32[:, d], j) for j in range(n_freq)], axis=1).astype(dt)
        cols += [np.cos(args), np.sin(args)]
    return np.concatenate(cols, axis=1)


def ray_points(top, bot, tvals):
    """the rays form's sample positions in the kernel's fp32 operation order: fl(fl(top * fl(1 - t)) + fl(bot * t))"""
    t = tvals.astype(np.float32)[None, :, None]
    omt = np.float32(1) - t
    return (top.astype(np.float32)[:, None, :] * omt + bot.astype(np.float32)[:, None, :] * t).reshape(-1, 3).astype(np.float32)


def ref_pe_points(v, par, dt):
    x = v["points"].astype(np.float32) if par["form"] == "points" else ray_points(v["top"], v["bot"], v["tvals"])
    pe = np.concatenate([pe_features(x, 10, dt), np.zeros((x.shape[0], 1), dtype=dt)], axis=1)
    out = {"pe": Out(pe, np.maximum(1.0, np.abs(pe.astype(np.float64))), "elem")}       # the three raw coordinates are not in [-1, 1]
    if "pe2" in v:
        out["pe2"] = out["pe"]
    if "pts" in v:
        out["pts"] = _elem(x.astype(dt))
    return out


def ref_pe_small(v, par, dt):
    D, F, stride = par["n_dims"], par["n_freq"], par["out_stride"]
    x = v["in"].astype(np.float32)[:, :D]
    pe = pe_features(x, F, dt)
    pe = np.concatenate([pe, np.zeros((x.shape[0], stride - pe.shape[1]), dtype=dt)], axis=1)
    return {"out": Out(pe, np.maximum(1.0, np.abs(pe.astype(np.float64))), "elem")}


def ref_softmax(v, par, dt):
    x = v["x"]
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return {"p": _elem(e / e.sum(axis=1, keepdims=True, dtype=dt), unit=True)}


def ref_softmax_bwd(v, par, dt):
    dot = np.sum(v["p"] * v["dp"], axis=1, keepdims=True, dtype=dt)
    dx = v["p"] * (v["dp"] - dot)
    # scale: the magnitude of the terms that meet in dp - dot, not of their difference
    return {"dx": Out(dx, np.abs(v["p"].astype(np.float64)) * (np.abs(v["dp"]) + np.sum(np.abs(v["p"] * v["dp"]), axis=1, keepdims=True)).astype(np.float64), "elem")}


def ref_sigmoid(v, par, dt):
    return {"y": _elem(_sigmoid(v["x"]), unit=True)}


def ref_sigmoid_bwd(v, par, dt):
    return {"dx": _elem(v["dy"] * v["y"] * (1 - v["y"]))}


def ref_colsum(v, par, dt):
    return {"out": _sum_out(v["X"], v["out"], par["alpha"])}


def ref_copy_cols(v, par, dt):
    return {"dst": _elem(v["dst"] + v["src"] if par["accumulate"] else v["src"])}


def ref_bcast_rows(v, par, dt):
    n, S, C, col0 = par["n"], par["n_samples"], par["C"], par["col0"]
    dst = v["dst"].copy()
    dst[:, col0:col0 + C] = v["src"][np.arange(n) // S]
    return {"dst": _elem(dst)}


def ref_reduce_rows(v, par, dt):
    G, S, C, col0 = par["G"], par["n_samples"], par["C"], par["col0"]
    t = v["src"][:, col0:col0 + C].reshape(G, S, C)
    val = np.sum(t, axis=1, dtype=dt)
    return {"dst": Out(val, np.sum(np.abs(t.astype(np.float64)), axis=1), "sum", t[:, 0], t[:, -1])}


def ref_fill(v, par, dt):
    return {"p": Out(np.zeros_like(v["p"]), np.zeros(v["p"].shape), "elem")}


def ref_copy(v, par, dt):
    return {"d": Out(v["s"].copy(), np.zeros(v["s"].shape), "elem")}


REFS = {k[4:]: f for k, f in list(globals().items()) if k.startswith("ref_")}


def evaluate(case, dt):
    """the case's reference in dtype dt (np.float64 / np.float32) on its fp32 inputs"""
    dt = np.dtype(dt)
    v = {b.name: (b.data.astype(dt) if b.data.dtype == np.float32 else b.data) for b in case.bufs if b is not None}      # double sums and bytes stay as they are
    with np.errstate(over="ignore", invalid="ignore"):
        return REFS[case.ref](v, case.par, dt)


def bounds(case):
    """{output: (float64 value, tolerance array, E_ref, Out)} of a case"""
    r64, r32 = evaluate(case, np.float64), evaluate(case, np.float32)
    res = {}
    for name, o in r64.items():
        val = np.asarray(o.value, dtype=np.float64)
        e_ref = float(np.max(np.abs(np.asarray(r32[name].value, dtype=np.float64) - val))) if val.size else 0.0
        res[name] = (val, tolerance(e_ref, np.asarray(o.scale, dtype=np.float64), o.factor), e_ref, o)
    return res


# ------------------------------------------------------------------------------------------------------------------ cases
def pow2_at_least(n):
    p = 1
    while p < n:
        p <<= 1
    return p


def vec_rows(C):
    """(rows of one pass, rows of one block) of colpass_vec_kernel for a short matrix: the launcher halves 512 while the grid stays under 512 blocks, down
    to 32 rows or one pass (tests/test_train_kernel_refs.py compares this with the launcher's own figure through the hook)"""
    rp = 256 // pow2_at_least(C // 4)
    return rp, max(32, rp)


def _mat(r, M, C, lo=-1.0, hi=1.0):
    return _f32(r.uniform(lo, hi, size=(M, C)))


def _bn_vectors(r, C):
    # no column that cancels: positive scale, every vector away from zero
    return {"mu": _f32(r.uniform(-.3, .3, C)), "istd": _f32(r.uniform(.6, 1.8, C)), "gamma": _f32(r.uniform(.5, 1.5, C) * r.choice([-1, 1], C)),
            "beta": _f32(r.uniform(-.5, .5, C))}


def _pad(C, k):
    """a leading dimension above C: the next multiple of 4 plus 4 k (vector shapes stay vector shapes), or an odd one for the scalar shapes"""
    return (C + 3) // 4 * 4 + 4 * k if C % 4 == 0 else C + 2 * k + 1


COL_VEC_C = [4, 12, 36, 64, 260, 1024]
COL_SCALAR_C = [18, 33, 130]


def _col_shapes():
    """(C, M, off, vec) of the column passes and sin_fwd"""
    out = []
    for C in COL_VEC_C:
        rp, rpb = vec_rows(C)
        for M in sorted({1, max(1, rp - 1), rpb - 1, rpb, rpb + 1, 1221}):
            out.append((C, M, 0, True))
    for C in COL_SCALAR_C:
        cp = 256 if C >= 256 else 128 if C >= 128 else 64 if C >= 64 else 32
        for M in sorted({1, 256 // cp - 1, 511, 512, 513, 1221}):
            out.append((C, M, 0, False))
    for M in (31, 513):
        out.append((64, M, 1, False))             # a vectorisable shape on a base 4 bytes off 16: the scalar kernels
    return out


def column_cases():
    cases = []
    for C, M, off, vec in _col_shapes():
        ld, ldd = _pad(C, 1), _pad(C, 2)
        tag = f"C{C}-M{M}" + ("-off" if off else "")
        for mode in (0, 1, 2):
            r = rng_for(f"colreduce{mode}-{tag}")
            bn = _bn_vectors(r, C)
            Z, D = _mat(r, M, C, -2, 2), _mat(r, M, C, .2, 1) * r.choice([-1, 1], (1, C)).astype(np.float32)
            o0, o1 = _f32(r.uniform(.5, 1.5, C)), _f32(r.uniform(-1.5, -.5, C))
            alpha = 30.0 if mode == 2 else 1.0
            bufs = [Buf("Z", Z, ld, "in", off), Buf("D", D, ldd, "inout", off) if mode else None] + \
                   [Buf(k, bn[k], None, "in") if mode != 2 else None for k in ("mu", "istd", "gamma", "beta")] + \
                   [Buf("out0", o0, None, "inout"), Buf("out1", o1, None, "inout") if mode == 1 else None]
            kern = "colreduce_kernel" if (mode == 0 or not vec) else f"colpass_vec_kernel<{mode}>"
            cases.append(Case(f"colreduce-m{mode}-{tag}", "colreduce", [mode, M, C, ld, ldd], [alpha], bufs, "colreduce", kern,
                              {"mode": mode, "alpha": alpha, "M": M, "C": C, "rows": ["Z", "D"]}))
        for d_is_dy, mg in ((0, 1), (1, 2)):
            r = rng_for(f"bn_bwd2-{d_is_dy}-{tag}")
            bn = _bn_vectors(r, C)
            Z, D = _mat(r, M, C, -2, 2), _mat(r, M, C, .2, 1)
            sdy, sdyx = _f32(r.uniform(-.2, .2, C) * mg * M), _f32(r.uniform(-.2, .2, C) * mg * M)
            bufs = [Buf("Z", Z, ld, "in", off), Buf("D", D, ldd, "inout", off)] + [Buf(k, bn[k], None, "in") for k in ("mu", "istd", "gamma", "beta")] + \
                   [Buf("sdy", sdy, None, "in"), Buf("sdyx", sdyx, None, "in"), Buf("dbias", _f32(r.uniform(.5, 1.5, C)), None, "inout")]
            kern = f"colpass_vec_kernel<{3 + d_is_dy}>" if vec else "bn_bwd2_kernel"
            cases.append(Case(f"bn_bwd2-dy{d_is_dy}-Mg{mg}-{tag}", "bn_bwd2", [M, C, ld, ldd, mg * M, d_is_dy], [30.0], bufs, "bn_bwd2", kern,
                              {"d_is_dy": d_is_dy, "M_global": mg * M, "alpha": 30.0, "M": M, "C": C, "rows": ["Z", "D"]}))
    return cases


def sin_cases():
    cases = []
    for C, M, off, vec in _col_shapes() + [(1024, 8200, 0, True)]:          # 8200 rows of one pass each: past the 8192-block cap
        for bn_on in ((1,) if M == 8200 else (0, 1)):
            tag = f"sin_fwd-bn{bn_on}-C{C}-M{M}" + ("-off" if off else "")
            r = rng_for(tag)
            bn = _bn_vectors(r, C)
            bufs = [Buf("Z", _mat(r, M, C, -3, 3), _pad(C, 1), "in", off), Buf("H", np.zeros((M, C), np.float32), _pad(C, 2), "out", off)] + \
                   [Buf(k, bn[k], None, "in") if bn_on else None for k in ("mu", "istd", "gamma", "beta")]
            cases.append(Case(tag, "sin_fwd", [M, C, _pad(C, 1), _pad(C, 2)], [], bufs, "sin_fwd", "sin_fwd_vec_kernel" if vec else "sin_fwd_kernel",
                              {"bn": bn_on, "M": M, "C": C, "rows": ["Z"]}))
    return cases


def finalizer_cases():
    cases = []
    for C in (1, 64, 260):
        for M in (1, 2, 1221):
            tag = f"C{C}-M{M}"
            r = rng_for("fin-" + tag)
            vec = lambda lo=-1.0, hi=1.0: _f32(r.uniform(lo, hi, C))
            for stage in (0, 1, 2):
                bufs = [Buf("colsum", vec(-M, M), None, "in") if stage == 0 else None, Buf("m2", vec(.1 * M, 2.0 * M), None, "in") if stage else None,
                        Buf("mean", vec(), None, "out" if stage == 0 else "in") if stage != 2 else None,
                        Buf("istd", np.zeros(C, np.float32), None, "out") if stage else None,
                        Buf("running_mean", vec(), None, "inout") if stage == 1 else None, Buf("running_var", vec(.5, 2), None, "inout") if stage == 1 else None]
                cases.append(Case(f"bn_finalize-s{stage}-{tag}", "bn_finalize", [M, C, stage], [], bufs, "bn_finalize", "bn_finalize_kernel",
                                  {"stage": stage, "M": M, "C": C, "rows": []}))
            for tab in (0, 1):
                alpha = 30.0
                bias = vec(-.05, .05)
                sigma = r.uniform(.5, 2, C)
                z = (alpha * bias.astype(np.float64))[None, :] + r.normal(size=(M, C)) * sigma + r.uniform(-1, 1, C)
                z[:, 0] = 0.75                                                  # a constant column: var_b clamps at 0
                if C > 1:
                    z[:, 1] += 1e3 * sigma[1]                                   # a mean 1e3 standard deviations from the shift
                zs = _f32(z).astype(np.float64) - (np.float32(alpha) * bias).astype(np.float64)
                stats = np.concatenate([zs.sum(0), (zs * zs).sum(0)])
                bufs = [Buf("stats", stats, None, "inout"), Buf("bias", bias, None, "in"), Buf("mean", np.zeros(C, np.float32), None, "out"),
                        Buf("istd", np.zeros(C, np.float32), None, "out"), Buf("running_mean", vec(), None, "inout"), Buf("running_var", vec(.5, 2), None, "inout"),
                        Buf("gamma", vec(.5, 1.5), None, "in") if tab else None, Buf("beta", vec(-.5, .5), None, "in") if tab else None,
                        Buf("tab", np.zeros(2 * C, np.float32), None, "out") if tab else None]
                cases.append(Case(f"bn_finalize_shifted-tab{tab}-{tag}", "bn_finalize_shifted", [M, C], [alpha], bufs, "bn_finalize_shifted",
                                  "bn_finalize_shifted_kernel", {"tab": tab, "alpha": alpha, "M": M, "C": C, "rows": []}))
        r = rng_for(f"actfin-{C}")
        vec = lambda lo=-1.0, hi=1.0: _f32(r.uniform(lo, hi, C))
        for full in (0, 1):
            bufs = [Buf("stats", r.uniform(-50, 50, 2 * C), None, "inout"), Buf("out0", np.zeros(C, np.float32), None, "out"),
                    Buf("out1", np.zeros(C, np.float32), None, "out") if full else None, Buf("acc0", vec(), None, "inout") if full else None,
                    Buf("acc1", vec(), None, "inout") if full else None]
            cases.append(Case(f"act_sums_finalize-full{full}-C{C}", "act_sums_finalize", [C], [30.0], bufs, "act_sums_finalize", "act_sums_finalize_kernel",
                              {"scale0": 30.0, "C": C, "rows": []}))
        for bn_on in (0, 1):
            bn = _bn_vectors(r, C)
            bufs = [Buf(k, bn[k], None, "in") if bn_on else None for k in ("mu", "istd", "gamma", "beta")] + [Buf("dst", np.zeros(2 * C, np.float32), None, "out")]
            cases.append(Case(f"act_table-bn{bn_on}-C{C}", "act_table", [C], [], bufs, "act_table", "act_table_kernel", {"bn": bn_on, "n": C, "rows": []}))
    return cases


def thin_rows(N):
    rp = 256 // pow2_at_least(N // 4)
    return rp, max(32, rp)


def thin_dgrad_cases():
    cases = []

    def add(N, M, K, ldd, acc, act, bn=0, w3=0):
        tag = f"thin_dgrad-N{N}-M{M}-K{K}-ldd{ldd}-acc{acc}-act{act}-bn{bn}-w3{w3}"
        r = rng_for(tag)
        ldw, ldc, eld = N + 4, N + 8, N + 12
        W = _mat(r, K, N, .2, 1) * r.choice([-1, 1], (K, N)).astype(np.float32)
        tab = np.concatenate([_f32(r.uniform(.05, .3, N)), _f32(r.uniform(-.5, .5, N))])
        D = _mat(r, M, K, .2, 1)
        if M > 100000:
            D[[0, -1]] *= 16          # one row in 2^18 of equal size is 16x the 2^-22 of the sum the tolerance allows at best: the edge rows carry more
        bufs = [Buf("D", D, ldd, "in"), Buf("W", W, ldw, "in"), Buf("W3", _mat(r, 1, N, .2, 1), None, "in") if w3 else None,
                Buf("C", _mat(r, M, N, .5, 1.5) if acc else np.zeros((M, N), np.float32), ldc, "inout" if acc else "out"),
                Buf("ez", _mat(r, M, N, -3, 3), eld, "in") if act else None, Buf("etab", tab, None, "in") if act else None,
                Buf("emu", _f32(r.uniform(-.3, .3, N)), None, "in") if bn else None, Buf("eistd", _f32(r.uniform(.6, 1.8, N)), None, "in") if bn else None,
                Buf("stats", r.uniform(.5, 1.5, 2 * N), None, "inout") if act else None]
        cases.append(Case(tag, "thin_dgrad", [M, N, K, ldd, ldw, ldc, acc, eld if act else 0], [0.5], bufs, "thin_dgrad",
                          "thin_dgrad_kernel<true>" if act else "thin_dgrad_kernel<false>",
                          {"K": K, "N": N, "M": M, "accumulate": acc, "act": act, "bn": bn, "w3": w3, "alpha": 0.5, "rows": ["D", "C", "ez"]}))

    i = 0
    for N in (4, 36, 128, 256, 1024):
        rp, chunk = thin_rows(N)
        for M in sorted({max(1, 4 * rp - 1), chunk - 1, chunk + 1, 3 * chunk + 5}):
            for K, ldd, w3 in ((1, 1, 0), (3, 4, 0), (4, 4, 0), (4, 6, 1), (3, 3, 0)):
                add(N, M, K, ldd, i % 2, (i // 2) % 2, bn=(i // 4) % 2 if (i // 2) % 2 else 0, w3=w3)
                i += 1
    for acc, act, bn in ((0, 0, 0), (1, 1, 1), (0, 1, 0)):
        add(8, 262144 + 77, 4 if act else 3, 4, acc, act, bn)          # more chunks than the 1024-block cap: the persistent loop
    return cases


def point_out_cases():
    cases = []
    edge = np.float32([-30, 19.99, 20.01, 60])
    for S in (1, 2, 7, 96, 300):
        for C in (1, 2, 3, 4, 5):
            R = {1: 517, 2: 300, 7: 111, 96: 7, 300: 3}[S] + C
            R += 1 if (R * S) % 256 == 0 else 0          # n is never a multiple of the block's 256 points
            n = R * S
            tag = f"S{S}-C{C}"
            r = rng_for("point_out-" + tag)
            head = _mat(r, n, 4, -3, 3)
            head[:: max(1, n // 40), 3] = np.resize(edge, len(head[:: max(1, n // 40)]))
            head[1:: max(1, n // 40), 0] = np.resize(edge, len(head[1:: max(1, n // 40)]))
            adj, sv_raw = _mat(r, n, 3 * C, .1, 1), _mat(r, n, 1, -4, 4)[:, 0]
            cls = _f32(r.dirichlet(np.ones(C), R)) if C > 1 else np.ones((R, 1), np.float32)
            z = lambda *s: np.zeros(s, np.float32)
            fwd = [Buf("head", head, None, "in"), Buf("adj", adj, None, "in"), Buf("sv_raw", sv_raw, None, "in"), Buf("cls", cls, None, "in"),
                   Buf("rho", z(n), None, "out"), Buf("col", z(n, 3), None, "out"), Buf("sv", z(n), None, "out"),
                   Buf("adjust_col", z(n, 3), None, "out") if C % 2 else None] + [None] * 7
            cases.append(Case(f"point_out_fwd-{tag}", "point_out_fwd", [n, S, C], [], fwd, "point_out_fwd", "point_out_fwd_kernel",
                              {"n_samples": S, "C": C, "rows": []}))
            col, sv = _mat(r, n, 3, .05, .95), _mat(r, n, 1, .05, .95)[:, 0]
            no_rho = C == 2
            bwd = [Buf("head", head, None, "in"), Buf("adj", adj, None, "in"), None, Buf("cls", cls, None, "in"), None, Buf("col", col, None, "in"),
                   Buf("sv", sv, None, "in"), None, None if no_rho else Buf("d_rho", _mat(r, n, 1, .2, 1)[:, 0], None, "in"),
                   Buf("d_col", _mat(r, n, 3, .2, 1), None, "in"), Buf("d_sv", _mat(r, n, 1, .2, 1)[:, 0], None, "in"), Buf("d_head", z(n, 4), None, "out"),
                   Buf("d_adj", z(n, 3 * C), None, "out"), Buf("d_cls", _mat(r, R, C, .5, 1.5), None, "inout"), Buf("d_sv_raw", z(n), None, "out")]
            cases.append(Case(f"point_out_bwd-{tag}", "point_out_bwd", [n, S, C], [], bwd, "point_out_bwd", "point_out_bwd_kernel",
                              {"n_samples": S, "C": C, "rows": []}))
        n = 5 * S + (0 if S > 1 else 300)
        r = rng_for(f"point_out-solar-S{S}")
        sv_raw = _mat(r, n, 1, -4, 4)[:, 0]
        cases.append(Case(f"point_out_fwd-solar-S{S}", "point_out_fwd", [n, S, 0], [], [None, None, Buf("sv_raw", sv_raw, None, "in"), None, None, None,
                          Buf("sv", np.zeros(n, np.float32), None, "out")] + [None] * 8, "point_out_fwd", "point_out_fwd_kernel", {"n_samples": S, "C": 0, "rows": []}))
        cases.append(Case(f"point_out_bwd-solar-S{S}", "point_out_bwd", [n, S, 0], [], [None] * 6 + [Buf("sv", _mat(r, n, 1, .05, .95)[:, 0], None, "in")] + [None] * 3 +
                          [Buf("d_sv", _mat(r, n, 1, .2, 1)[:, 0], None, "in")] + [None] * 3 + [Buf("d_sv_raw", np.zeros(n, np.float32), None, "out")],
                          "point_out_bwd", "point_out_bwd_kernel", {"n_samples": S, "C": 0, "rows": []}))
    return cases


PE_EDGE = np.float32([0.0, -0.0, 1, -1, 1 - 2.0 ** -24, -(1 - 2.0 ** -24), 2.5, -2.5, 1e3, -1e3])


def encoding_cases():
    cases = []
    for form in ("points", "rays"):
        for extra in (0, 1):
            tag = f"pe_points-{form}-x{extra}"
            r = rng_for(tag)
            S = 7
            R = 41
            n = R * S
            if form == "points":
                pts = _mat(r, n, 3)
                pts[:len(PE_EDGE)] = PE_EDGE[:, None]
                for d in range(3):
                    pts[30 + d * len(PE_EDGE):30 + (d + 1) * len(PE_EDGE), d] = PE_EDGE
                src = [Buf("points", pts, None, "in"), None, None, None]
            else:
                top, bot = _mat(r, R, 3), _mat(r, R, 3)
                top[:len(PE_EDGE), 0] = PE_EDGE
                bot[:len(PE_EDGE), 0] = PE_EDGE
                top[:len(PE_EDGE), 2] = PE_EDGE[::-1]
                tv = _f32(np.linspace(0, 1, S))
                src = [None, Buf("top", top, None, "in"), Buf("bot", bot, None, "in"), Buf("tvals", tv, None, "in")]
            ld2 = 64 + 12
            z = lambda *s: np.zeros(s, np.float32)
            bufs = src + [Buf("pe", z(n, 64), None, "out"), Buf("pts", z(n, 3), None, "out") if extra else None, Buf("pe2", z(n, 64), ld2, "out") if extra else None]
            cases.append(Case(tag, "pe_points", [n, S, ld2 if extra else 0], [], bufs, "pe_points", "pe_points_kernel", {"form": form, "rows": []}))
    for name, in_cols, D, F, stride in (("sun", 3, 3, 4, 28), ("time", 4, 2, 2, 12)):
        for rows in (1, 257):
            r = rng_for(f"pe_small-{name}-{rows}")
            x = _mat(r, rows, in_cols)
            x[:min(rows, len(PE_EDGE)), 0] = PE_EDGE[:min(rows, len(PE_EDGE))]
            x[:min(rows, len(PE_EDGE)), D - 1] = PE_EDGE[::-1][:min(rows, len(PE_EDGE))]
            bufs = [Buf("in", x, None, "in"), Buf("out", np.zeros((rows, stride), np.float32), None, "out")]
            cases.append(Case(f"pe_small-{name}-r{rows}", "pe_small", [rows, in_cols, D, F, stride], [], bufs, "pe_small", "pe_small_kernel",
                              {"n_dims": D, "n_freq": F, "out_stride": stride, "rows": []}))
    return cases


SMALL_ROWS = [1, 255, 256, 257, 1025]


def small_cases():
    cases = []
    z = lambda *s: np.zeros(s, np.float32)
    for n in SMALL_ROWS:
        r = rng_for(f"small-{n}")
        C = 4
        x = _mat(r, n, C, -4, 4)
        cases.append(Case(f"softmax-r{n}", "softmax", [n, C], [], [Buf("x", x, None, "in"), Buf("p", z(n, C), None, "out")], "softmax", "softmax_kernel", {"rows": []}))
        p = _f32(r.dirichlet(np.ones(C), n))
        cases.append(Case(f"softmax_bwd-r{n}", "softmax_bwd", [n, C], [], [Buf("p", p, None, "in"), Buf("dp", _mat(r, n, C, .2, 1), None, "in"), Buf("dx", z(n, C), None, "out")],
                          "softmax_bwd", "softmax_bwd_kernel", {"rows": []}))
        cases.append(Case(f"sigmoid-n{n}", "sigmoid", [n], [], [Buf("x", x[:, 0].copy(), None, "in"), Buf("y", z(n), None, "out")], "sigmoid", "sigmoid_kernel", {"rows": []}))
        cases.append(Case(f"sigmoid_bwd-n{n}", "sigmoid_bwd", [n], [], [Buf("y", _mat(r, n, 1, .05, .95)[:, 0], None, "in"), Buf("dy", _mat(r, n, 1, .2, 1)[:, 0], None, "in"),
                          Buf("dx", z(n), None, "out")], "sigmoid_bwd", "sigmoid_bwd_kernel", {"rows": []}))
        for acc in (0, 1):
            C2 = 5
            cases.append(Case(f"copy_cols-acc{acc}-r{n}", "copy_cols", [n, C2, C2 + 3, C2 + 6, acc], [], [Buf("src", _mat(r, n, C2), C2 + 3, "in"),
                              Buf("dst", _mat(r, n, C2), C2 + 6, "inout" if acc else "out")], "copy_cols", "copy_cols_kernel", {"accumulate": acc, "M": n, "C": C2, "rows": ["src", "dst"]}))
        S, C3, col0, ldp = 3, 4, 2, 9
        cases.append(Case(f"bcast_rows-g{n}", "bcast_rows", [n * S, S, C3, ldp, col0], [], [Buf("src", _mat(r, n, C3), None, "in"), Buf("dst", _mat(r, n * S, ldp - 1), ldp, "inout")],
                          "bcast_rows", "bcast_rows_kernel", {"n": n * S, "n_samples": S, "C": C3, "col0": col0, "rows": []}))
        cases.append(Case(f"reduce_rows-g{n}", "reduce_rows", [n, S, C3, ldp, col0], [], [Buf("src", _mat(r, n * S, ldp - 1, .2, 1), ldp, "in"), Buf("dst", z(n, C3), None, "out")],
                          "reduce_rows", "reduce_rows_kernel", {"G": n, "n_samples": S, "C": C3, "col0": col0, "rows": []}))
    for C in (1, 12, 16, 17, 33):
        for M in SMALL_ROWS:
            r = rng_for(f"colsum-{C}-{M}")
            cases.append(Case(f"colsum-C{C}-M{M}", "colsum", [M, C, C + 3], [30.0], [Buf("X", _mat(r, M, C, .2, 1) * r.choice([-1, 1], (1, C)).astype(np.float32), C + 3, "in"),
                              Buf("out", _f32(r.uniform(.5, 1.5, C)), None, "inout")], "colsum", "colsum_kernel", {"alpha": 30.0, "M": M, "C": C, "rows": ["X"]}))
    for n in (1024, 1025, 1026, 1027, 3):
        for off in (0, 1):
            r = rng_for(f"fill-{n}-{off}")
            cases.append(Case(f"fill_zero-n{n}-off{off}", "fill_zero", [n], [], [Buf("p", _mat(r, 1, n)[0], None, "inout", off)], "fill", "fill_zero_kernel", {"rows": []}))
            cases.append(Case(f"copy_f32-n{n}-off{off}", "copy_f32", [n], [], [Buf("d", z(n), None, "out", off), Buf("s", _mat(r, 1, n)[0], None, "in", off)], "copy", "copy_f32_kernel", {"rows": []}))
            b8 = r.integers(0, 256, 4 * n - 1 - 2 * off).astype(np.uint8)          # odd byte counts, bases 0 and 1 byte off
            cases.append(Case(f"fill_zero_bytes-n{b8.size}-off{off}", "fill_zero_bytes", [b8.size], [], [Buf("p", b8, None, "inout", off)], "fill", "fill_zero_bytes_kernel", {"rows": []}))
            cases.append(Case(f"copy_bytes-n{b8.size}-off{off}", "copy_bytes", [b8.size], [], [Buf("d", np.zeros_like(b8), None, "out", off), Buf("s", b8, None, "in", 1 - off)], "copy", "copy_bytes_kernel", {"rows": []}))
            cases.append(Case(f"copy_f32-n{n}-mixed{off}", "copy_f32", [n], [], [Buf("d", z(n), None, "out", off), Buf("s", _mat(r, 1, n)[0], None, "in", 1 - off)], "copy", "copy_f32_kernel", {"rows": []}))
    return cases


_ALL = None


def all_cases():
    global _ALL
    if _ALL is None:
        _ALL = column_cases() + sin_cases() + finalizer_cases() + thin_dgrad_cases() + point_out_cases() + encoding_cases() + small_cases()
        ids = [c.id for c in _ALL]
        assert len(ids) == len(set(ids))
    return _ALL
