"""Cases and float64 references for the weight gradients of the training engine, run through snerf_train_kernel_debug: the ten instances of
wgrad_bf16x3_kernel<FULL, BNZ, TA, TB> with their two reductions, two stage orders, the BatchNorm ride and run_wgrad's two-launch split ("wgrad"),
and the two-head form of the thin heads' streams ("thin_wgrad", "thin_fwd").  Shared by tests/test_gpu_wgrad_instances.py (the kernels against
these references on the GPU) and tests/test_wgrad_refs.py (the references against torch.autograd, the conditions that keep the cases honest and
the routing through dry runs, on the CPU).  Built on tests/train_kernel_cases.py: the same Buf / Case / Out, the same tolerance rule.

References (evaluated in a dtype dt: float64 the yardstick, float32 the measure E of what fp32 arithmetic costs on these inputs):
    wgrad       xhat = (z - mu) istd;  dZ = gamma istd (dY - sdy / Mg - xhat sdyx / Mg)   (without the BatchNorm block: dZ is the input, read-only)
                H = In, sin(2 pi (a In + b)) over the first tab_cols columns;  dW += alpha dZ^T H;  dbias += bias_alpha sum_m dZ;  the dZ buffer holds dZ
    thin_wgrad  dW[k] += alpha D[:, k]^T H  for k < K, row 3 into dW3 where that is given (dW's own row 3 then stays as it was)
    thin_fwd    Out[m, k] = alpha (sum_n H[m, n] W[k, n] + bias[k]), row 3 of W and element 3 of bias from W3 / bias3 where given

Tolerance: FACTOR * (E + 2^-24 * scale), FACTOR = 4, as everywhere.  For dW on the MFMA kernel E is the sum of two CPU quantities: the fp32
evaluation's deviation from float64, and the deviation of the three-term split product (hi = bf16(x), lo = bf16(x - hi), hi hi + hi lo + lo hi, every
term exact, summed in float64) from the float64 product of the same fp32 operands - the algorithm's own error, no property of the kernel under test.
No output has a wider margin: see DBIAS_FACTOR below for the one that was examined.
"""
from collections import namedtuple

import numpy as np

import train_kernel_cases as tk
from train_kernel_cases import Buf, Case, Out, FACTOR, rng_for, _f32, _sum_out, _elem

# The kernels the hook's new operations report (csrc/train.h TrainKernel, include/season_nerf_hip.h)
WGRAD_KERNELS = {"wgrad<F,F,1,2>": 30, "wgrad<F,T,1,2>": 31, "wgrad<F,F,2,2>": 32, "wgrad<F,T,2,2>": 33, "wgrad<F,F,1,4>": 34, "wgrad<F,T,1,4>": 35,
                 "wgrad<F,F,2,4>": 36, "wgrad<F,T,2,4>": 37, "wgrad<T,F,2,4>": 38, "wgrad<T,T,2,4>": 39}
THIN_KERNELS = {"thin_wgrad_kernel<false>": 40, "thin_wgrad_kernel<true>": 41, "thin_fwd_kernel<false>": 42, "thin_fwd_kernel<true>": 43}
KERNEL_NAMES = {v: k for k, v in {**WGRAD_KERNELS, **THIN_KERNELS}.items()}

# dbias of the ride: a lane adds the 16 rows it gathers per stage into one fp32 chain over all stages of its workgroup, the two half-waves meet in one
# addition, and every workgroup's sum reaches dbias through an fp32 atomic - a second chain, over the row blocks, in whatever order they finish - where the
# fp32 reference adds pairwise.  The column passes' sums needed a wider margin for such a chain (train_kernel_cases.CHAIN_FACTOR: 256 additions in a row);
# here the chains are short (16 rows per stage, at most 8 stages per workgroup at the sizes of the list, 206 atomics at 32845 rows), and emulate_dbias
# below - that order on the CPU, in fp32 from the float64 terms, row blocks ascending and descending - measures at most 0.47 of the FACTOR = 4 tolerance
# over the case list (tests/test_wgrad_refs.py prints and asserts it): no wider margin, dbias is held to FACTOR like everything else.
DBIAS_FACTOR = FACTOR

Launch = namedtuple("Launch", "kernel partial reverse")


def unpack(rc):
    """the "wgrad" operation's return value -> its one or two launches: per byte kernel | partial << 6 | reverse << 7, the second byte 0 for one launch"""
    out = [Launch(rc & 63, (rc >> 6) & 1, (rc >> 7) & 1)]
    if rc >> 8:
        out.append(Launch((rc >> 8) & 63, (rc >> 14) & 1, (rc >> 15) & 1))
    return out


def plan(M, n_out, n_in, cus=256):
    """the launcher's rule (csrc/gemm.hip plan_wgrad_bf16x3), stated a second time: (ta, tb, (bx, by, bz), rows per block, partial)"""
    ta, tb = (1 if n_out <= 128 else 2), (2 if n_in <= 128 else 4)
    bo, bi = 128 * ta, 64 * tb
    by, bz = -(-n_out // bo), -(-n_in // bi)
    bx = max(1, max(8, cus // 8 * 8) // (by * bz))
    rows = max(128, -(-(-(-M // bx)) // 32) * 32)
    bx = -(-M // rows)
    return ta, tb, (bx, by, bz), rows, int(bx >= 8 and 2 * min(n_out, bo) * min(n_in, bi) >= bo * bi)


def expected_launches(par, cus=256):
    """[(kernel number, partial)] of a wgrad case: one launch, or run_wgrad's split of a BatchNorm layer with more than 256 inputs"""
    M, n_out, n_in, bn = par["M"], par["n_out"], par["n_in"], par["bn"]
    parts = [(256, bn), (n_in - 256, 0)] if bn and n_in > 256 else [(n_in, bn)]
    out = []
    for (ni, ride), name in zip(parts, par["inst"]):
        out.append((WGRAD_KERNELS[name], plan(M, n_out, ni, cus)[4]))
    return out


# ------------------------------------------------------------------------------------------------------------------ references
def bf16(x):
    """float32 -> the nearest bfloat16 (ties to even), as float32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def split3_product(A32, B32):
    """A^T B by the kernel's algorithm in exact arithmetic: hi = bf16(x), lo = bf16(x - hi), hi hi + hi lo + lo hi, summed in float64"""
    ah, bh = bf16(A32), bf16(B32)
    al, bl = bf16(A32 - ah), bf16(B32 - bh)
    d = np.float64
    return ah.astype(d).T @ bh.astype(d) + ah.astype(d).T @ bl.astype(d) + al.astype(d).T @ bh.astype(d)


def activated(In, tab, tab_cols, dt, tab_b=None):
    """H: In with sin(2 pi (a In + b)) over the first tab_cols columns; tab = [a | b] (tab_b: the b half, where a corruption reads it elsewhere)"""
    H = In.copy()
    if tab_cols:
        a, b = tab[:tab_cols], (tab[tab_cols:2 * tab_cols] if tab_b is None else tab_b)
        H[:, :tab_cols] = np.sin(dt.type(2 * np.pi) * (a * In[:, :tab_cols] + b))
    return H


def bn_dz(v, par, dt):
    xh = (v["z"] - v["mu"]) * v["istd"]
    mg = dt.type(par["M_global"])
    return (v["gamma"] * v["istd"]) * (v["dZ"] - v["sdy"] / mg - xh * (v["sdyx"] / mg))


def wgrad_operands(v, par, dt):
    """the two factors of the product: dZ (through the BatchNorm backward where the case has the block) and H"""
    return (bn_dz(v, par, dt) if par["bn"] else v["dZ"]), activated(v["In"], v.get("tab"), par["tab_cols"], dt, v.get("tab_b"))


def ref_wgrad(v, par, dt):
    dz, H = wgrad_operands(v, par, dt)
    alpha = dt.type(par["alpha"])
    dW = v["dW"] + alpha * (dz.T @ H)
    scale = np.abs(v["dW"].astype(np.float64)) + abs(par["alpha"]) * (np.abs(dz.astype(np.float64)).T @ np.abs(H.astype(np.float64)))
    out = {"dW": Out(dW, scale, "sum", alpha * np.outer(dz[0], H[0]), alpha * np.outer(dz[-1], H[-1]))}
    if par["bn"]:
        out["dZ"] = _elem(dz)
        if "dbias" in v:
            out["dbias"] = _sum_out(dz, v["dbias"], par["bias_alpha"], DBIAS_FACTOR)
    return out


def split_error(case):
    """the three-term split product's deviation from the float64 product of the same fp32 operands, times |alpha|: the algorithm's own error on this case"""
    dz, H = wgrad_operands(inputs(case, np.dtype(np.float32)), case.par, np.dtype(np.float32))
    return float(abs(case.par["alpha"]) * np.max(np.abs(split3_product(dz, H) - dz.astype(np.float64).T @ H.astype(np.float64))))


def ref_thin_wgrad(v, par, dt):
    K = par["K"]
    H = activated(v["In"], v.get("tab"), par["tab_cols"], dt)
    D = v["D"][:, :K]
    alpha = dt.type(par["alpha"])
    prod = alpha * (D.T @ H)                                             # [K, N]
    scale = abs(par["alpha"]) * (np.abs(D.astype(np.float64)).T @ np.abs(H.astype(np.float64)))
    first, last = alpha * np.outer(D[0], H[0]), alpha * np.outer(D[-1], H[-1])
    two = "dW3" in v and not par.get("row3_into_dW")                     # (row3_into_dW: the corruption of tests/test_wgrad_refs.py)
    keep = np.ones((K, 1)) if not two else (np.arange(K) != 3).astype(np.float64)[:, None]
    k = keep.astype(dt)
    out = {"dW": Out(v["dW"] + k * prod, np.abs(v["dW"].astype(np.float64)) + keep * scale, "sum", k * first, k * last)}
    if "dW3" in v:
        t = dt.type(1 if two else 0)
        out["dW3"] = Out(v["dW3"] + t * prod[3:4], np.abs(v["dW3"].astype(np.float64)) + scale[3:4], "sum", t * first[3:4], t * last[3:4])
    return out


def ref_thin_fwd(v, par, dt):
    K = par["K"]
    H = activated(v["In"], v.get("tab"), par["tab_cols"], dt)
    W, bias = v["W"][:K].copy(), v["bias"][:K].copy()
    if "W3" in v:
        W[3] = v["W3"][0]
    if "bias3" in v:
        bias[3] = v["bias3"][0]
    alpha = dt.type(par["alpha"])
    val = alpha * (H @ W.T + bias)
    scale = abs(par["alpha"]) * (np.abs(H.astype(np.float64)) @ np.abs(W.astype(np.float64)).T + np.abs(bias.astype(np.float64)))
    return {"Out": Out(val, scale, "elem")}


REFS = {"wgrad": ref_wgrad, "thin_wgrad": ref_thin_wgrad, "thin_fwd": ref_thin_fwd}


def inputs(case, dt, override=None):
    v = {b.name: b.data.astype(dt) for b in case.bufs if b is not None}
    v.update(override or {})
    return v


def evaluate(case, dt, override=None, par=None):
    dt = np.dtype(dt)
    with np.errstate(over="ignore", invalid="ignore"):
        return REFS[case.ref](inputs(case, dt, override), par or case.par, dt)


_BOUNDS = {}


def bounds(case):
    """{output: (float64 value, tolerance array, E, Out)} of a case (kept: the references of the large cases are computed once per process)"""
    if case.id in _BOUNDS:
        return _BOUNDS[case.id]
    r64, r32 = evaluate(case, np.float64), evaluate(case, np.float32)
    res = {}
    for name, o in r64.items():
        val = np.asarray(o.value, dtype=np.float64)
        e = float(np.max(np.abs(np.asarray(r32[name].value, dtype=np.float64) - val))) if val.size else 0.0
        if case.op == "wgrad" and name == "dW":
            e += split_error(case)
        res[name] = (val, tk.tolerance(e, np.asarray(o.scale, dtype=np.float64), o.factor), e, o)
    _BOUNDS[case.id] = res
    return res


def emulate_dbias(terms64, init32, bias_alpha, bx, reverse=False, block_order=None):
    """dbias as wgrad_bf16x3_kernel<., true, ., .> adds it up, in fp32 from the float64 terms dZ [M, C]: 32-row stages dealt round-robin over bx workgroups;
    per column two lanes (rows 0-7 + 16-23 and 8-15 + 24-31 of a stage) each one chain over the workgroup's stages, one addition of the two, times
    bias_alpha, then one atomic per workgroup onto dbias in block_order (default: ascending)."""
    M, C = terms64.shape
    t = terms64.astype(np.float32)
    n_total = -(-M // 32)
    out = init32.astype(np.float32).copy()
    for x in (block_order if block_order is not None else range(bx)):
        stages = list(range(x, n_total, bx))
        if reverse:
            stages.reverse()
        lane = np.zeros((2, C), dtype=np.float32)
        for s in stages:
            for h in (0, 1):
                for ks in (0, 1):
                    for e in range(8):
                        m = s * 32 + h * 8 + ks * 16 + e
                        if m < M:
                            lane[h] = lane[h] + t[m]
        if stages:
            out = out + np.float32(bias_alpha) * (lane[0] + lane[1])
    return out


# ------------------------------------------------------------------------------------------------------------------ cases
# (instance of the first launch without its BNZ letter, n_out, n_in, BatchNorm ride possible).  n_in > 256 without the ride: two blocks over the inputs.
SHAPES = [("1,2", 64, 64, 1), ("1,2", 37, 100, 1), ("1,2", 128, 128, 1), ("1,2", 12, 128, 1),
          ("2,2", 256, 128, 1), ("2,2", 200, 63, 1),
          ("1,4", 128, 256, 1), ("1,4", 100, 200, 1), ("1,4", 64, 319, 0),
          ("2,4", 200, 200, 1), ("2,4", 319, 256, 1), ("2,4", 256, 319, 0),
          ("F", 256, 256, 1), ("F", 512, 256, 1), ("F", 256, 512, 0), ("F", 512, 512, 0)]
PRIMARY = {(64, 64), (200, 63), (100, 200), (200, 200), (256, 256)}          # one shape per block shape takes every row count
ROWS = [1, 31, 32, 33, 127, 128, 129, 897, 2049]
ROWS_FEW = [[33, 897], [1, 897, 129], [32, 897, 2049], [127, 897, 31], [128, 897]]
# run_wgrad's split: (n_out, n_in, tab_cols, (first instance, second instance))
SPLITS = [(256, 319, 256, ("wgrad<T,T,2,4>", "wgrad<F,F,2,2>")), (256, 319, 319, ("wgrad<T,T,2,4>", "wgrad<F,F,2,2>")),
          (512, 512, 512, ("wgrad<T,T,2,4>", "wgrad<T,F,2,4>")), (512, 576, 512, ("wgrad<T,T,2,4>", "wgrad<F,F,2,4>")),
          (256, 319, 100, ("wgrad<T,T,2,4>", "wgrad<F,F,2,2>")), (256, 319, 0, ("wgrad<T,T,2,4>", "wgrad<F,F,2,2>"))]
BIG_M = 32768 + 77
# one per block shape, all on the partial-sum route at this row count: (n_out, n_in, ride, tab_cols)
BIG = [(128, 128, 1, 128), (256, 128, 0, 84), (100, 200, 1, 200), (200, 200, 0, 0), (256, 256, 1, 169)]


def inst_name(shape, bn):
    return f"wgrad<T,{'T' if bn else 'F'},2,4>" if shape == "F" else f"wgrad<F,{'T' if bn else 'F'},{shape}>"


def wgrad_case(n_out, n_in, M, bn, tab_cols, inst, mg=1):
    cid = f"wgrad-o{n_out}-i{n_in}-M{M}-bn{bn}-tab{tab_cols}"
    r = rng_for(cid)
    ldz, ldi, ldw, ldzz = n_out + 3, n_in + 5, n_in + 2, n_out + 7          # all above their column counts, no two alike
    assert len({ldz, ldi, ldw, ldzz}) == 4, cid
    u = lambda lo, hi, *s: _f32(r.uniform(lo, hi, s))
    dY = u(.2, 1, M, n_out) * r.choice([-1, 1], (M, n_out)).astype(np.float32)
    In = u(-1, 1, M, n_in)
    if tab_cols:
        In[:, :tab_cols] = u(-3, 3, M, tab_cols)
    tab = np.concatenate([u(.05, .3, tab_cols), u(-.5, .5, tab_cols)]) if tab_cols else None
    alpha = 30.0 if bn else 0.5
    bufs = [Buf("dZ", dY, ldz, "inout" if bn else "in"), Buf("In", In, ldi, "in"), Buf("dW", u(.5, 1.5, n_out, n_in), ldw, "inout"),
            Buf("tab", tab, None, "in") if tab_cols else None]
    if bn:
        # per-column statistics that differ from their neighbours' (a kernel that took column c + 1's must miss), no column that cancels
        vec = {"gamma": u(.5, 1.5, n_out) * r.choice([-1, 1], n_out).astype(np.float32), "mu": u(-.3, .3, n_out), "istd": u(.6, 1.8, n_out),
               "sdy": u(-.2, .2, n_out) * np.float32(mg * M), "sdyx": u(-.2, .2, n_out) * np.float32(mg * M)}
        bufs += [Buf("z", u(-2, 2, M, n_out), ldzz, "in")] + [Buf(k, vec[k], None, "in") for k in ("gamma", "mu", "istd", "sdy", "sdyx")] + \
                [Buf("dbias", u(.5, 1.5, n_out), None, "inout")]
    else:
        bufs += [None] * 7
    sizes = [M, n_out, n_in, ldz, ldi, ldw, tab_cols, ldzz if bn else 0, mg * M if bn else 0, 1]
    par = {"M": M, "n_out": n_out, "n_in": n_in, "bn": bn, "tab_cols": tab_cols, "alpha": alpha, "bias_alpha": 30.0, "M_global": mg * M, "inst": inst,
           "ldz": ldz, "ldi": ldi}
    return Case(cid, "wgrad", sizes, [alpha, 30.0], bufs, "wgrad", inst, par)


def wgrad_cases():
    cases = []
    for si, (shape, n_out, n_in, can_bn) in enumerate(SHAPES):
        rows = ROWS if (n_out, n_in) in PRIMARY else ROWS_FEW[si % len(ROWS_FEW)]
        for mi, M in enumerate(rows):
            for bn in ((0, 1) if can_bn else (0,)):
                # with the table: over every column, or over a leading part that ends inside a 32-column tile
                for tab_cols in (0, n_in if (si + mi) % 2 == 0 else max(1, n_in * 2 // 3 - 1)):
                    cases.append(wgrad_case(n_out, n_in, M, bn, tab_cols, (inst_name(shape, bn),), mg=1 + (si + mi) % 2))
    for si, (n_out, n_in, tab_cols, inst) in enumerate(SPLITS):
        for M in (33, 897, 2049):
            cases.append(wgrad_case(n_out, n_in, M, 1, tab_cols, inst, mg=1 + si % 2))
    return cases


def big_cases():
    """one case per block shape at 32768 + 77 rows (the stage order alternates from 32768 rows on; the last stage holds 13 rows), with and without the ride"""
    shape_of = {(o, i): s for s, o, i, _ in SHAPES}
    return [wgrad_case(n_out, n_in, BIG_M, bn, tab_cols, (inst_name(shape_of[(n_out, n_in)], bn),)) for n_out, n_in, bn, tab_cols in BIG]


def thin_wgrad_case(N, M, K, ldd, two, tab_cols, d_off=0):
    cid = f"thin_wgrad-N{N}-M{M}-K{K}-ldd{ldd}-two{two}-tab{tab_cols}-off{d_off}"
    r = rng_for(cid)
    u = lambda lo, hi, *s: _f32(r.uniform(lo, hi, s))
    ldi, ldw = N + 4, N + 3
    In = u(-1, 1, M, N)
    if tab_cols:
        In[:, :tab_cols] = u(-3, 3, M, tab_cols)
    tab = np.concatenate([u(.05, .3, tab_cols), u(-.5, .5, tab_cols)]) if tab_cols else None
    D = u(.2, 1, M, K) * r.choice([-1, 1], (M, K)).astype(np.float32)
    bufs = [Buf("D", D, ldd, "in", d_off), Buf("In", In, ldi, "in"), Buf("dW", u(.5, 1.5, K, N), ldw, "inout"),
            Buf("dW3", u(-1.5, -.5, 1, N), None, "inout") if two else None, Buf("tab", tab, None, "in") if tab_cols else None]
    par = {"M": M, "N": N, "K": K, "alpha": 0.5, "tab_cols": tab_cols, "two": two}
    return Case(cid, "thin_wgrad", [M, N, K, ldd, ldi, ldw, tab_cols], [0.5], bufs, "thin_wgrad",
                "thin_wgrad_kernel<true>" if tab_cols else "thin_wgrad_kernel<false>", par)


def thin_fwd_case(N, M, K, two, tab_cols):
    cid = f"thin_fwd-N{N}-M{M}-K{K}-two{two}-tab{tab_cols}"
    r = rng_for(cid)
    u = lambda lo, hi, *s: _f32(r.uniform(lo, hi, s))
    ldi, ldw, ldo = N + 4, N + 3, K + 2
    In = u(-1, 1, M, N)
    if tab_cols:
        In[:, :tab_cols] = u(-3, 3, M, tab_cols)
    tab = np.concatenate([u(.05, .3, tab_cols), u(-.5, .5, tab_cols)]) if tab_cols else None
    W = u(.2, 1, K, N) * r.choice([-1, 1], (K, N)).astype(np.float32) / np.float32(np.sqrt(N))
    bufs = [Buf("In", In, ldi, "in"), Buf("W", W, ldw, "in"), Buf("W3", u(.2, 1, 1, N) / np.float32(np.sqrt(N)), None, "in") if two else None,
            Buf("bias", u(.5, 1.5, K), None, "in"), Buf("bias3", u(-1.5, -.5, 1), None, "in") if two else None,
            Buf("Out", np.zeros((M, K), np.float32), ldo, "out"), Buf("tab", tab, None, "in") if tab_cols else None]
    par = {"M": M, "N": N, "K": K, "alpha": 1.5, "tab_cols": tab_cols, "two": two}
    return Case(cid, "thin_fwd", [M, N, K, ldi, ldw, ldo, tab_cols], [1.5], bufs, "thin_fwd",
                "thin_fwd_kernel<true>" if tab_cols else "thin_fwd_kernel<false>", par)


THIN_N = [12, 64, 128, 256, 1024]
THIN_WGRAD_CAP_M = 512 * 16 + 77        # N = 1024: 16 rows per block, 512 blocks at most - a block walks more than one chunk
THIN_FWD_CAP_M = 2048 * 16 + 77         # N = 256: 16 rows per block, 2048 blocks at most


def thin_cases():
    cases = []
    for N in THIN_N:
        part = max(1, N * 2 // 3 - 1)
        for M in [7, 1025] + ([THIN_WGRAD_CAP_M] if N == 1024 else []):
            for tab_cols in (0, N, part):
                cases.append(thin_wgrad_case(N, M, 4, 4, 1, tab_cols))                       # two heads, D as 16-byte rows
            cases.append(thin_wgrad_case(N, M, 4, 4, 1, part, d_off=1))                      # ... D off its 16 bytes: the scalar gather
            cases.append(thin_wgrad_case(N, M, 4, 6, 1, 0))                                  # ... ldd no multiple of 4: the scalar gather
            cases.append(thin_wgrad_case(N, M, 4, 4, 0, N))                                  # one address for all four rows
            cases.append(thin_wgrad_case(N, M, 3, 4, 0, 0))
            cases.append(thin_wgrad_case(N, M, 1, 1, 0, part))
        if N <= 256:
            for M in [7, 1025] + ([THIN_FWD_CAP_M] if N == 256 else []):
                for tab_cols in (0, N, part):
                    cases.append(thin_fwd_case(N, M, 4, 1, tab_cols))
                cases.append(thin_fwd_case(N, M, 4, 0, part))
                cases.append(thin_fwd_case(N, M, 3, 0, 0))
                cases.append(thin_fwd_case(N, M, 1, 0, N))
    return cases


_ALL = {}


def all_cases():
    if not _ALL:
        _ALL["cases"] = wgrad_cases() + thin_cases()
        ids = [c.id for c in _ALL["cases"]]
        assert len(ids) == len(set(ids))
    return _ALL["cases"]
