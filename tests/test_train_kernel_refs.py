"""CPU checks of tests/train_kernel_cases.py, so that the float64 references of tests/test_gpu_train_kernels.py are not their own judge and its
case list cannot pass a kernel that is wrong at a tail:
  - every backward formula against torch.autograd in float64 on the corresponding forward, the encodings against oracle.pe_encode;
  - every reduction case: the reference with the first row left out, with the last row left out and with the last row counted twice misses the
    case's tolerance by at least 10x in some column;
  - every elementwise case with a row stride: the reference that reads its inputs with ld and C swapped fails;
  - the case list names every kernel variant, and its row counts sit where the launchers' own block sizes put the edges."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import train_kernel_cases as tk
from oracle import season_nerf_oracle as orc

CASES = tk.all_cases()


def test_case_list_names_every_kernel_variant():
    assert {c.kernel for c in CASES} == set(tk.KERNELS)
    assert sorted(tk.KERNELS.values()) == list(range(30))
    thin = [c.par for c in CASES if c.op == "thin_dgrad"]
    for N in (4, 36, 128, 256, 1024):                        # every width meets every form of the call
        mine = [p for p in thin if p["N"] == N]
        assert {(p["act"], p["bn"]) for p in mine} == {(0, 0), (1, 0), (1, 1)} and {p["accumulate"] for p in mine} == {0, 1}
        assert {p["K"] for p in mine} == {1, 3, 4} and {p["w3"] for p in mine} == {0, 1}
    ldds = {(c.sizes[3], c.par["K"]) for c in CASES if c.op == "thin_dgrad"}
    assert (1, 1) in ldds and (4, 4) in ldds and (4, 3) in ldds       # scalar loads of D, 16-byte loads, 16-byte loads with a column past K
    assert {c.par["C"] for c in CASES if c.op.startswith("point_out") and c.par["C"]} == {1, 2, 3, 4, 5}
    assert {c.par["n_samples"] for c in CASES if c.op.startswith("point_out")} == {1, 2, 7, 96, 300}
    assert all(c.sizes[0] % 256 for c in CASES if c.op.startswith("point_out"))


def test_reduction_cases_notice_a_row_left_out_or_counted_twice():
    n = 0
    for case in CASES:
        for name, (val, tol, e_ref, o) in tk.bounds(case).items():
            if o.kind != "sum":
                continue
            n += 1
            # value - first, value - last, value + last: the reference without its first row, without its last row, with its last row twice
            for what, term in (("first", o.first), ("last", o.last)):
                miss = np.abs(np.asarray(term, dtype=np.float64)).reshape(val.shape) / np.maximum(tol, 1e-300)
                assert miss.max() >= 10, f"{case.id} {name}: leaving the {what} row out moves no column by 10x the tolerance (largest {miss.max():.2f}x)"
    assert n > 300


STRIDED_OPS = {"colreduce", "bn_bwd2", "sin_fwd", "thin_dgrad", "copy_cols"}


def test_elementwise_cases_notice_swapped_ld_and_C():
    """a kernel that walked its rows with stride C instead of ld (row r read at r * C) must fail every elementwise case with at least two rows; row 0
    does not depend on the stride, so the one-row cases cannot tell - each operation has cases with more rows"""
    seen = set()
    for case in CASES:
        rows = [b for b in case.bufs if b is not None and b.name in case.par["rows"] and b.role != "out" and b.ld not in (None, b.data.shape[1])]
        if not rows or rows[0].data.shape[0] < 2:
            continue
        want = tk.bounds(case)
        if not any(o.kind == "elem" for _, _, _, o in want.values()):
            continue
        r = tk.rng_for("swap-" + case.id)
        swapped = []
        for b in case.bufs:
            if b in rows:
                M, Cc = b.data.shape
                flat = r.uniform(.2, 1, M * b.ld).astype(np.float32)
                flat.reshape(M, b.ld)[:, :Cc] = b.data
                b = b._replace(data=flat[:M * Cc].reshape(M, Cc).copy())
            swapped.append(b)
        wrong = tk.evaluate(case._replace(bufs=swapped), np.float64)
        failed = False
        for name, (val, tol, _, o) in want.items():
            if o.kind == "elem":
                failed |= bool((np.abs(np.asarray(wrong[name].value, dtype=np.float64) - val) > tol).any())
        assert failed, case.id
        seen.add(case.op)
    assert seen == STRIDED_OPS


@pytest.fixture(scope="module")
def lib():
    import season_nerf_amd as sn
    return sn._lib.lib()


def _rows_per_block(lib, op, M, C_):
    s = (C.c_int64 * 2)(M, C_)
    return lib.snerf_train_kernel_debug(op.encode(), s, 2, None, 0, None, 0, None)


def test_row_counts_sit_at_the_launchers_block_edges(lib):
    """the cases' row counts come from vec_rows / thin_rows; the launchers' own figures (no launch: the hook returns them) must agree at every case"""
    n = 0
    for case in CASES:
        if case.kernel.startswith("colpass_vec_kernel"):
            assert _rows_per_block(lib, "colpass_rows_per_block", case.par["M"], case.par["C"]) == tk.vec_rows(case.par["C"])[1], case.id
            n += 1
        if case.op == "thin_dgrad" and case.par["M"] < 100000:
            assert _rows_per_block(lib, "thin_dgrad_rows_per_block", case.par["M"], case.par["N"]) == tk.thin_rows(case.par["N"])[1], case.id
            n += 1
    assert n > 200
    for C_ in tk.COL_VEC_C:
        rp, rpb = tk.vec_rows(C_)
        ms = {c.par["M"] for c in CASES if c.kernel == "colpass_vec_kernel<3>" and c.par["C"] == C_}
        assert {1, max(1, rp - 1), rpb - 1, rpb, rpb + 1, 1221} <= ms          # one row, below one pass, around one block, several blocks
    assert _rows_per_block(lib, "thin_dgrad_rows_per_block", 262144 + 77, 8) == 256 and (262144 + 77 + 255) // 256 > 1024      # more chunks than blocks


# ------------------------------------------------------------------------------------------------------------------ references against autograd
def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


def _close(a, b, what):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), b.detach().numpy(), rtol=1e-9, atol=1e-12, err_msg=what)


def test_sine_backward_references_match_autograd():
    r = tk.rng_for("autograd-sine")
    M, Cc = 37, 6
    z, dH = r.normal(size=(M, Cc)), r.normal(size=(M, Cc))
    gamma, beta = r.uniform(.5, 1.5, Cc), r.normal(size=Cc)
    # plain layer (mode 2): H = sin(z + bias), the bias gradient is the column sum scaled by alpha
    zt = _t(z, True)
    (torch.sin(zt) * _t(dH)).sum().backward()
    out = tk.ref_colreduce({"Z": z, "D": dH, "out0": np.zeros(Cc)}, {"mode": 2, "alpha": 30.0}, np.dtype(np.float64))
    _close(out["D"].value, zt.grad, "mode 2 dZ")
    _close(out["out0"].value, 30.0 * zt.grad.sum(0), "mode 2 bias sum")
    # BatchNorm layer: H = sin(gamma * xhat + beta) on batch statistics; modes 0 / 1 and the second pass
    zt = _t(z, True)
    mean, var = zt.mean(0), zt.var(0, unbiased=False)
    (torch.sin(_t(gamma) * (zt - mean) / torch.sqrt(var + 1e-5) + _t(beta)) * _t(dH)).sum().backward()
    mu = z.mean(0)
    m2 = tk.ref_colreduce({"Z": z, "mu": mu, "out0": np.zeros(Cc)}, {"mode": 0}, np.dtype(np.float64))["out0"].value
    _close(m2 / M, var, "mode 0 variance")
    istd = 1 / np.sqrt(m2 / M + 1e-5)
    bn = {"Z": z, "mu": mu, "istd": istd, "gamma": gamma, "beta": beta}
    s = tk.ref_colreduce({**bn, "D": dH, "out0": np.zeros(Cc), "out1": np.zeros(Cc)}, {"mode": 1}, np.dtype(np.float64))
    sums = {"sdy": s["out0"].value, "sdyx": s["out1"].value, "dbias": np.zeros(Cc)}
    out = tk.ref_bn_bwd2({**bn, **sums, "D": dH}, {"d_is_dy": 0, "M_global": M, "alpha": 30.0}, np.dtype(np.float64))
    _close(out["D"].value, zt.grad, "BatchNorm dZ")
    _close(out["dbias"].value, 30.0 * zt.grad.sum(0), "BatchNorm bias sum")
    dy = dH * np.cos(gamma * (z - mu) * istd + beta)
    out2 = tk.ref_bn_bwd2({**bn, **sums, "D": dy}, {"d_is_dy": 1, "M_global": M, "alpha": 30.0}, np.dtype(np.float64))
    _close(out2["D"].value, zt.grad, "BatchNorm dZ from dY")
    # the forward itself and the finalisers' statistics
    H = tk.ref_sin_fwd(bn, {"bn": 1}, np.dtype(np.float64))["H"].value
    _close(H, torch.sin(_t(gamma) * (_t(z) - mean) / torch.sqrt(var + 1e-5) + _t(beta)), "sin(BN(z))")


def test_finaliser_references_match_batchnorm():
    r = tk.rng_for("autograd-bn")
    for M in (1, 2, 50):
        Cc = 5
        z = r.normal(size=(M, Cc)) * 2 + 3
        bias, alpha = r.normal(size=Cc).astype(np.float32), 30.0
        shift = (np.float32(alpha) * bias).astype(np.float64)
        zs = z - shift
        rm, rv = r.normal(size=Cc), r.uniform(.5, 2, Cc)
        gamma, beta = r.uniform(.5, 1.5, Cc), r.normal(size=Cc)
        v = {"stats": np.concatenate([zs.sum(0), (zs * zs).sum(0)]), "bias": bias.astype(np.float64), "running_mean": rm, "running_var": rv, "gamma": gamma, "beta": beta}
        out = tk.ref_bn_finalize_shifted(v, {"C": Cc, "M": M, "alpha": alpha, "tab": 1}, np.dtype(np.float64))
        bn = torch.nn.BatchNorm1d(Cc, eps=1e-5, momentum=0.01).double()
        with torch.no_grad():
            bn.running_mean.copy_(_t(rm)); bn.running_var.copy_(_t(rv)); bn.weight.copy_(_t(gamma)); bn.bias.copy_(_t(beta))
        if M > 1:
            y = bn.train()(_t(z))
            np.testing.assert_allclose(out["running_mean"].value, bn.running_mean.numpy(), rtol=1e-9)
            np.testing.assert_allclose(out["running_var"].value, bn.running_var.numpy(), rtol=1e-7)
            a, b = out["tab"].value[:Cc], out["tab"].value[Cc:]
            np.testing.assert_allclose(np.sin(2 * np.pi * (a * z + b)), torch.sin(y).detach().numpy(), atol=1e-7)      # the [a | b] table is the BatchNorm
        else:                                                                        # one row: the biased variance (0) feeds the running estimate
            np.testing.assert_allclose(out["running_var"].value, 0.99 * rv, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(out["mean"].value, z.mean(0), rtol=1e-9)
        np.testing.assert_allclose(out["istd"].value, 1 / np.sqrt(z.var(0) + 1e-5), rtol=1e-6)
        # the two-pass finaliser states the same statistics
        st1 = tk.ref_bn_finalize({"m2": ((z - z.mean(0)) ** 2).sum(0), "mean": z.mean(0), "running_mean": rm, "running_var": rv}, {"stage": 1, "M": M}, np.dtype(np.float64))
        np.testing.assert_allclose(st1["istd"].value, out["istd"].value, rtol=1e-6)
        np.testing.assert_allclose(st1["running_var"].value, out["running_var"].value, rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(st1["running_mean"].value, out["running_mean"].value, rtol=1e-9)


def test_thin_dgrad_reference_matches_autograd():
    r = tk.rng_for("autograd-thin")
    M, N, K = 23, 8, 4
    z, D, W, W3 = r.normal(size=(M, N)), r.normal(size=(M, K)), r.normal(size=(K, N)), r.normal(size=(1, N))
    tab = np.concatenate([r.uniform(.05, .3, N), r.uniform(-.5, .5, N)])
    mu, istd = r.normal(size=N), r.uniform(.5, 2, N)
    base = r.normal(size=(M, N))
    Wt = W.copy(); Wt[3] = W3[0]
    arg = _t(2 * np.pi * (tab[:N] * z + tab[N:]), True)
    Hb = torch.sin(arg)                                             # the layer below; the head reads alpha * H W^T; `base` is another consumer's dL/dH
    Hb.retain_grad()
    ((0.5 * Hb @ _t(Wt).T) * _t(D)).sum().add((Hb * _t(base)).sum()).backward()
    par = {"K": K, "N": N, "alpha": 0.5, "accumulate": 1, "w3": 1, "act": 0, "bn": 0}
    v = {"D": D, "W": W, "W3": W3, "C": base, "ez": z, "etab": tab, "emu": mu, "eistd": istd, "stats": np.ones(2 * N)}
    _close(tk.ref_thin_dgrad(v, par, np.dtype(np.float64))["C"].value, Hb.grad, "dL/dH")
    out = tk.ref_thin_dgrad(v, {**par, "act": 1, "bn": 1}, np.dtype(np.float64))
    _close(out["C"].value, arg.grad, "dL/d(arg)")
    xh = (z - mu) * istd
    _close(out["stats"].value, torch.cat([1 + arg.grad.sum(0), 1 + (arg.grad * _t(xh)).sum(0)]), "column sums")
    assert np.all(tk.ref_thin_dgrad(v, {**par, "act": 1, "bn": 0}, np.dtype(np.float64))["stats"].value[N:] == 1)      # no BatchNorm below: xhat is 0


def test_point_output_references_match_autograd():
    r = tk.rng_for("autograd-point")
    S, Cc, R = 5, 3, 4
    n = R * S
    head = r.normal(size=(n, 4)) * 3
    head[:4, 3] = [-30, 19.99, 20.01, 60]
    adj, sv_raw, cls = r.normal(size=(n, 3 * Cc)), r.normal(size=n), r.dirichlet(np.ones(Cc), R)
    d_rho, d_col, d_sv = r.normal(size=n), r.normal(size=(n, 3)), r.normal(size=n)
    ht, at, st, ct = _t(head, True), _t(adj, True), _t(sv_raw, True), _t(cls, True)
    rho = torch.nn.functional.softplus(ht[:, 3], threshold=20)
    ac = torch.einsum("ick,ic->ik", at.view(n, Cc, 3), ct.repeat_interleave(S, 0))
    col, sv = torch.sigmoid(ht[:, :3] + ac), torch.sigmoid(st)
    z = np.zeros
    fwd = tk.ref_point_out_fwd({"head": head, "adj": adj, "sv_raw": sv_raw, "cls": cls, "rho": z(n), "col": z((n, 3)), "sv": z(n), "adjust_col": z((n, 3))},
                               {"n_samples": S, "C": Cc}, np.dtype(np.float64))
    for k, t in (("rho", rho), ("col", col), ("sv", sv), ("adjust_col", ac)):
        _close(fwd[k].value, t, k)
    ((rho * _t(d_rho)).sum() + (col * _t(d_col)).sum() + (sv * _t(d_sv)).sum()).backward()
    init = r.normal(size=(R, Cc))
    bwd = tk.ref_point_out_bwd({"head": head, "adj": adj, "cls": cls, "col": fwd["col"].value, "sv": fwd["sv"].value, "d_rho": d_rho, "d_col": d_col, "d_sv": d_sv,
                                "d_head": z((n, 4)), "d_adj": z((n, 3 * Cc)), "d_cls": init, "d_sv_raw": z(n)}, {"n_samples": S, "C": Cc}, np.dtype(np.float64))
    _close(bwd["d_head"].value, ht.grad, "d_head")
    _close(bwd["d_adj"].value, at.grad, "d_adj")
    _close(bwd["d_cls"].value - init, ct.grad, "d_cls")
    _close(bwd["d_sv_raw"].value, st.grad, "d_sv_raw")


def test_softmax_and_sigmoid_references_match_autograd():
    r = tk.rng_for("autograd-soft")
    x, dp = r.normal(size=(9, 4)) * 3, r.normal(size=(9, 4))
    xt = _t(x, True)
    p = torch.softmax(xt, 1)
    (p * _t(dp)).sum().backward()
    pv = tk.ref_softmax({"x": x}, {}, np.dtype(np.float64))["p"].value
    _close(pv, p, "softmax")
    _close(tk.ref_softmax_bwd({"p": pv, "dp": dp}, {}, np.dtype(np.float64))["dx"].value, xt.grad, "softmax backward")
    xt = _t(x, True)
    y = torch.sigmoid(xt)
    (y * _t(dp)).sum().backward()
    yv = tk.ref_sigmoid({"x": x}, {}, np.dtype(np.float64))["y"].value
    _close(yv, y, "sigmoid")
    _close(tk.ref_sigmoid_bwd({"y": yv, "dy": dp}, {}, np.dtype(np.float64))["dx"].value, xt.grad, "sigmoid backward")


def test_encoding_references_match_the_oracle():
    """oracle.pe_encode on fp32 input forms fl32(x * fl32(pi/2 * 2^j)) - the kernels' argument exactly (a power of two commutes with the rounding) - and takes
    its sine and cosine in fp32: within 2 ulp of 1 of the float64 functions of that argument"""
    r = tk.rng_for("oracle-pe")
    x = np.concatenate([np.repeat(tk.PE_EDGE[:, None], 3, 1), r.uniform(-1, 1, (200, 3)).astype(np.float32)])
    for n_freq in (10, 4, 2):
        ref = tk.pe_features(x, n_freq, np.dtype(np.float64))
        o = orc.pe_encode(torch.from_numpy(x), n_freq).numpy().astype(np.float64)
        assert ref.shape == o.shape
        assert np.abs(ref - o).max() <= 2 * 2.0 ** -23
    case = next(c for c in CASES if c.id == "pe_points-points-x1")
    pe = tk.evaluate(case, np.float64)["pe"].value
    pts = case.bufs[0].data
    assert pe.shape == (pts.shape[0], 64) and np.all(pe[:, 63] == 0)
    assert np.abs(pe[:, :63] - orc.pe_encode(torch.from_numpy(pts), 10).numpy()).max() <= 2 * 2.0 ** -23
    for cid, D, F, width in (("pe_small-sun-r257", 3, 4, 27), ("pe_small-time-r257", 2, 2, 10)):
        case = next(c for c in CASES if c.id == cid)
        out = tk.evaluate(case, np.float64)["out"].value
        assert np.all(out[:, width:] == 0) and out.shape[1] == width + (1 if D == 3 else 2)
        assert np.abs(out[:, :width] - orc.pe_encode(torch.from_numpy(case.bufs[0].data[:, :D].copy()), F).numpy()).max() <= 2 * 2.0 ** -23
    # the rays form: positions as the oracle's sampler forms them
    case = next(c for c in CASES if c.id == "pe_points-rays-x1")
    top, bot, tv = (torch.from_numpy(case.bufs[i].data) for i in (1, 2, 3))
    p = (top[:, None, :] * (1 - tv)[None, :, None] + bot[:, None, :] * tv[None, :, None]).reshape(-1, 3).numpy()
    np.testing.assert_array_equal(tk.evaluate(case, np.float64)["pts"].value, p.astype(np.float64))
    assert math.isclose(float(tk.HALF_PI32), math.pi / 2, rel_tol=1e-7)
