"""CPU checks of tests/wgrad_cases.py, so that the float64 references of tests/test_gpu_wgrad_instances.py are not their own judge and its case list
cannot pass a kernel that is wrong at an edge:
  - the BatchNorm reference against torch.autograd of a float64 Linear + BatchNorm layer (dZ, dW, and dbias = bias_alpha x the bias gradient), the
    thin references against autograd of the two heads, the split reference (two products over column windows) against the unsplit one;
  - for every case, each corruption a wrong index would cause misses the case's tolerance by at least 10x on some element: the first or last row left
    out or counted twice (dW, dbias, dZ), ldz swapped with ldi, the table window of the split's second launch shifted by n0 or its b half read at
    stride in_cols instead of tab_cols, mu or istd taken from the neighbouring column, row 3 of the two-head product written into dW;
  - the order in which the ride adds dbias up, emulated from float64 terms, against the tolerance the case list gives it (DBIAS_FACTOR = FACTOR: no wider margin);
  - the routing, through dry runs of the hook (no GPU: the CU count falls back to 256): every case lands on the instance and the reduction it names,
    the list reaches all ten instances, both reductions and the split, a dry run takes no turn of the direction, and the weight gradients the engine
    issues at W = 64, 256 and 512 - from the layer table of csrc/train.cpp - land on covered instances."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import train_kernel_cases as tk
import wgrad_cases as wc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = wc.all_cases()
BIG = wc.big_cases()
WGRAD = [c for c in CASES + BIG if c.op == "wgrad"]
F64 = np.dtype(np.float64)


def test_case_list_names_every_instance_and_edge():
    assert {n for c in WGRAD for n in c.kernel} == set(wc.WGRAD_KERNELS)
    assert {c.kernel for c in CASES if c.op != "wgrad"} == set(wc.THIN_KERNELS)
    assert sorted({**wc.WGRAD_KERNELS, **wc.THIN_KERNELS}.values()) == list(range(30, 44)) and max(tk.KERNELS.values()) == 29
    shapes = {(c.par["n_out"], c.par["n_in"]) for c in WGRAD}
    assert shapes >= {(o, i) for _, o, i, _ in wc.SHAPES} | {(o, i) for o, i, _, _ in wc.SPLITS}
    for o, i in wc.PRIMARY:
        assert {c.par["M"] for c in WGRAD if (c.par["n_out"], c.par["n_in"]) == (o, i)} >= set(wc.ROWS)
    for _, o, i, can_bn in wc.SHAPES:          # every shape that can carry the ride runs with and without it, and with and without a table
        mine = [c.par for c in CASES if c.op == "wgrad" and (c.par["n_out"], c.par["n_in"]) == (o, i) and len(c.par["inst"]) == 1]
        assert {p["bn"] for p in mine} == ({0, 1} if can_bn else {0}) and {bool(p["tab_cols"]) for p in mine} == {False, True}
        assert 897 in {p["M"] for p in mine}
    assert any(len(c.par["inst"]) == 2 and 0 < c.par["tab_cols"] < 256 for c in WGRAD) and any(len(c.par["inst"]) == 2 and c.par["tab_cols"] > 256 for c in WGRAD)
    thin = [c for c in CASES if c.op == "thin_wgrad"]
    assert {c.par["N"] for c in thin if c.par["two"]} == set(wc.THIN_N) and {c.par["N"] for c in CASES if c.op == "thin_fwd" and c.par["two"]} == {12, 64, 128, 256}
    assert any(c.bufs[0].off for c in thin) and any(c.sizes[3] % 4 for c in thin)                         # the scalar gather of D, both ways
    assert any(c.par["M"] > 512 * 16 and c.par["N"] == 1024 for c in thin) and any(c.par["M"] == 1025 for c in thin)
    for c in CASES + BIG:                       # no two leading dimensions of a wgrad case alike, every one above its column count
        if c.op == "wgrad":
            lds = [b.ld for b in c.bufs if b is not None and b.ld is not None]
            assert len(lds) == len(set(lds)) and all(b.ld > b.data.shape[1] for b in c.bufs if b is not None and b.ld is not None), c.id


# ------------------------------------------------------------------------------------------------------------------ references against autograd
def _t(a, grad=False):
    return torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=grad)


def _close(a, b, what):
    np.testing.assert_allclose(np.asarray(a, dtype=np.float64), b.detach().numpy(), rtol=1e-9, atol=1e-11, err_msg=what)


def test_batchnorm_reference_matches_autograd():
    r = tk.rng_for("autograd-wgrad")
    M, n_in, n_out, tc = 41, 9, 6, 5
    alpha = 30.0
    In, W, b = r.normal(size=(M, n_in)), r.normal(size=(n_out, n_in)) * .1, r.normal(size=n_out) * .1
    tab = np.concatenate([r.uniform(.05, .3, tc), r.uniform(-.5, .5, tc)])
    gamma, beta, dY = r.uniform(.5, 1.5, n_out), r.normal(size=n_out), r.normal(size=(M, n_out))
    H = wc.activated(In, tab, tc, F64)
    Wt, bt = _t(W, True), _t(b, True)
    z = alpha * (_t(H) @ Wt.T + bt)                                        # the SineLayer's Linear: z = 30 (H W^T + b)
    mean, var = z.mean(0), z.var(0, unbiased=False)
    istd = 1 / torch.sqrt(var + 1e-5)
    xh = (z - mean) * istd
    z.retain_grad()
    ((_t(gamma) * xh + _t(beta)) * _t(dY)).sum().backward()               # dY: dL/d(BatchNorm output)
    dW0, db0 = r.normal(size=(n_out, n_in)), r.normal(size=n_out)
    v = {"dZ": dY, "z": z.detach().numpy(), "mu": mean.detach().numpy(), "istd": istd.detach().numpy(), "gamma": gamma, "sdy": dY.sum(0),
         "sdyx": (dY * xh.detach().numpy()).sum(0), "In": In, "tab": tab, "dW": dW0, "dbias": db0}
    out = wc.ref_wgrad(v, {"bn": 1, "tab_cols": tc, "alpha": alpha, "bias_alpha": alpha, "M_global": M}, F64)
    _close(out["dZ"].value, z.grad, "dZ")
    _close(out["dW"].value - dW0, Wt.grad, "dW")
    _close(out["dbias"].value - db0, bt.grad, "dbias = bias_alpha x the bias gradient")
    # without the block: dZ is what it is given
    out = wc.ref_wgrad({"dZ": dY, "In": In, "dW": dW0}, {"bn": 0, "tab_cols": 0, "alpha": .5}, F64)
    _close(out["dW"].value - dW0, .5 * _t(dY).T @ _t(In), "plain dW")
    assert set(out) == {"dW"}


def test_thin_references_match_autograd():
    r = tk.rng_for("autograd-thin-heads")
    M, N, tc = 29, 8, 5
    In, D = r.normal(size=(M, N)), r.normal(size=(M, 4))
    tab = np.concatenate([r.uniform(.05, .3, tc), r.uniform(-.5, .5, tc)])
    Wc, Wd, bc, bd = (_t(r.normal(size=s), True) for s in ((3, N), (1, N), (3,), (1,)))          # colour head rows 0..2, density head row 3
    H = _t(wc.activated(In, tab, tc, F64))
    out = 1.5 * torch.cat([H @ Wc.T + bc, H @ Wd.T + bd], 1)
    W4 = np.concatenate([Wc.detach().numpy(), np.full((1, N), 99.0)])                            # row 3 / element 3 of the first address: never read
    f = wc.ref_thin_fwd({"In": In, "tab": tab, "W": W4, "W3": Wd.detach().numpy(), "bias": np.append(bc.detach().numpy(), 99.0), "bias3": bd.detach().numpy()},
                        {"K": 4, "alpha": 1.5, "tab_cols": tc}, F64)
    _close(f["Out"].value, out, "two-head forward")
    (out * _t(D)).sum().backward()
    dW0, dW30 = r.normal(size=(4, N)), r.normal(size=(1, N))
    g = wc.ref_thin_wgrad({"D": D, "In": In, "tab": tab, "dW": dW0, "dW3": dW30}, {"K": 4, "alpha": 1.5, "tab_cols": tc}, F64)
    _close(g["dW"].value[:3] - dW0[:3], Wc.grad, "colour head dW")
    _close(g["dW3"].value - dW30, Wd.grad, "density head dW")
    assert np.array_equal(g["dW"].value[3], dW0[3])
    one = wc.ref_thin_wgrad({"D": D, "In": In, "tab": tab, "dW": dW0}, {"K": 4, "alpha": 1.5, "tab_cols": tc}, F64)
    _close(one["dW"].value[3:] - dW0[3:], Wd.grad, "one address: row 3 in dW")


def _windows(case, v, par):
    """the split as run_wgrad issues it: the first 256 input columns with the block, the rest on the finished dZ; each with its window of the table"""
    n0, tc = 256, par["tab_cols"]
    a, b = (v["tab"][:tc], v["tab"][tc:]) if tc else (None, None)
    c0 = min(tc, n0)
    v0 = {**v, "In": v["In"][:, :n0], "dW": v["dW"][:, :n0], "tab": np.concatenate([a[:c0], b[:c0]]) if c0 else None}
    first = wc.ref_wgrad(v0, {**par, "tab_cols": c0, "n_in": n0}, F64)
    rest = max(0, tc - n0)
    v1 = {"dZ": first["dZ"].value, "In": v["In"][:, n0:], "dW": v["dW"][:, n0:], "tab": np.concatenate([a[n0:], b[n0:]]) if rest else None}
    second = wc.ref_wgrad(v1, {**par, "bn": 0, "tab_cols": rest, "n_in": par["n_in"] - n0}, F64)
    return first, second


def test_split_reference_equals_the_unsplit_one():
    n = 0
    for case in WGRAD:
        if len(case.par["inst"]) != 2 or case.par["M"] > 900:
            continue
        v = wc.inputs(case, F64)
        whole = wc.ref_wgrad(v, case.par, F64)
        first, second = _windows(case, v, case.par)
        np.testing.assert_allclose(np.concatenate([first["dW"].value, second["dW"].value], 1), whole["dW"].value, rtol=1e-12, atol=1e-12)
        np.testing.assert_array_equal(first["dZ"].value, whole["dZ"].value)
        np.testing.assert_array_equal(first["dbias"].value, whole["dbias"].value)
        n += 1
    assert n >= 10


# ------------------------------------------------------------------------------------------------------------------ the conditions
def _restride(data, ld, ld_wrong, r):
    """the [M, C] matrix a reader with the wrong row stride sees in the buffer that holds `data` at stride ld (padding: finite filler)"""
    M, Cc = data.shape
    flat = r.uniform(.2, 1, M * max(ld, ld_wrong) + Cc)
    flat[:M * ld].reshape(M, ld)[:, :Cc] = data
    return np.lib.stride_tricks.as_strided(flat, (M, Cc), (8 * ld_wrong, 8)).copy()


def _misses(want, wrong, names, least=10.0):
    worst = 0.0
    for name in names:
        val, tol, _, _ = want[name]
        worst = max(worst, float(np.max(np.abs(np.asarray(wrong[name].value, dtype=np.float64) - val) / np.maximum(tol, 1e-300))))
    return worst >= least, worst


def _light(case):
    """the conditions recompute the product per corruption: the 32845-row cases on their first 24 output columns (an element that misses is an element)"""
    if case.par["M"] <= 4000:
        return case
    k = 24
    cut = {"dZ", "z", "gamma", "mu", "istd", "sdy", "sdyx", "dbias"}
    bufs = [b if b is None or b.name not in cut | {"dW"} else b._replace(data=np.ascontiguousarray(b.data[:k] if b.name == "dW" else b.data[..., :k])) for b in case.bufs]
    return case._replace(id=case.id + "-light", bufs=bufs, par={**case.par, "n_out": k})


def test_every_case_notices_a_wrong_index():
    n = {"row": 0, "ld": 0, "shift": 0, "stride": 0, "mu": 0, "istd": 0, "row3": 0}
    for full in CASES + BIG:
        case = _light(full)
        want = wc.bounds(case)
        # a row left out or counted twice: the reductions by the row's own term, the in-place dZ by holding dY where dZ belongs
        for name, (val, tol, _, o) in want.items():
            if o.kind != "sum" or (name == "dW" and case.op == "thin_wgrad" and case.par["two"] and not np.any(o.first)):
                continue
            for what, term in (("first", o.first), ("last", o.last)):
                miss = np.abs(np.asarray(term, dtype=np.float64)).reshape(val.shape) / np.maximum(tol, 1e-300)
                assert miss.max() >= 10, f"{case.id} {name}: the {what} row left out moves no element by 10x the tolerance ({miss.max():.2f}x)"
            n["row"] += 1
        if case.op == "thin_fwd":
            continue
        v = wc.inputs(case, F64)
        r = tk.rng_for("wrong-" + case.id)
        if case.op == "thin_wgrad":
            if case.par["two"]:
                ok, worst = _misses(want, wc.evaluate(case, F64, par={**case.par, "row3_into_dW": 1}), ["dW", "dW3"])
                assert ok, f"{case.id}: row 3 written into dW ({worst:.2f}x)"
                n["row3"] += 1
            continue
        par = case.par
        if par["bn"]:
            dY = v["dZ"]
            for row in (0, -1):
                miss = np.abs(dY[row] - want["dZ"][0][row]) / want["dZ"][1][row]
                assert miss.max() >= 10, f"{case.id}: dZ row {row} not written ({miss.max():.2f}x)"
            for key in ("mu", "istd"):
                ok, worst = _misses(want, wc.evaluate(case, F64, {key: np.roll(v[key], -1)}), ["dW", "dZ", "dbias"])
                assert ok, f"{case.id}: {key} of the neighbouring column ({worst:.2f}x)"
                n[key] += 1
        if par["M"] >= 2:              # (row 0 does not depend on the stride)
            wrong = wc.evaluate(case, F64, {"dZ": _restride(v["dZ"], par["ldz"], par["ldi"], r), "In": _restride(v["In"], par["ldi"], par["ldz"], r)})
            ok, worst = _misses(want, wrong, ["dW"])
            assert ok, f"{case.id}: ldz swapped with ldi ({worst:.2f}x)"
            n["ld"] += 1
        tc = par["tab_cols"]
        if len(par["inst"]) == 2 and tc > 256:
            a, b = v["tab"][:tc], v["tab"][tc:]
            rest = tc - 256
            shifted = np.concatenate([a[:256], a[:rest], b[:256], b[:rest]])                                # the second launch reads the first window's entries
            ok, worst = _misses(want, wc.evaluate(case, F64, {"tab": shifted}), ["dW"])
            assert ok, f"{case.id}: table window not shifted by n0 ({worst:.2f}x)"
            flat = v["tab"]
            tab_b = np.concatenate([flat[256:512], flat[256 + rest:256 + 2 * rest]])                        # b at distance in_cols (256, rest) from a, not tab_cols
            ok, worst = _misses(want, wc.evaluate(case, F64, {"tab_b": tab_b}), ["dW"])
            assert ok, f"{case.id}: b half read at stride in_cols ({worst:.2f}x)"
            n["shift"] += 1
            n["stride"] += 1
    print(n)
    assert n["row"] > 400 and n["ld"] > 250 and n["mu"] > 100 and n["istd"] > 100 and n["shift"] >= 6 and n["row3"] >= 40


def test_dbias_summation_order_fits_its_margin():
    """emulate_dbias - the ride's order of additions in fp32 from float64 terms, row blocks in ascending and in descending order, stages forwards and
    backwards - stays inside DBIAS_FACTOR x (E + 2^-24 scale) on every shape it is tried on; its largest fraction of the FACTOR = 4 tolerance is printed"""
    worst4 = 0.0
    for case in WGRAD:
        par = case.par
        if not par["bn"] or len(par["inst"]) != 1 or par["M"] not in (897, 2049, wc.BIG_M):
            continue
        if par["M"] == wc.BIG_M:
            case = _light(case)
        val, tol, e, o = wc.bounds(case)["dbias"]
        v = wc.inputs(case, F64)
        bx = wc.plan(par["M"], par["n_out"], par["n_in"])[2][0]
        dz = wc.bn_dz(v, par, F64)
        init = next(b.data for b in case.bufs if b is not None and b.name == "dbias")
        for reverse, order in ((False, None), (True, list(range(bx))[::-1])):
            got = wc.emulate_dbias(dz, init, par["bias_alpha"], bx, reverse, order).astype(np.float64)
            frac = float(np.max(np.abs(got - val) / tol))
            worst4 = max(worst4, frac * wc.DBIAS_FACTOR / wc.FACTOR)
            assert frac <= 1, (case.id, frac)
    print(f"dbias in the kernel's order: at most {worst4:.3f} of the FACTOR = 4 tolerance")


# ------------------------------------------------------------------------------------------------------------------ routing, through dry runs
FAKE = 1 << 24


@pytest.fixture(scope="module")
def lib():
    import season_nerf_amd as sn
    L = sn._lib.lib()
    assert L.snerf_rows_debug_set(None, 1, 0) == 0          # dry run: plan, record, launch nothing
    yield L
    assert L.snerf_rows_debug_set(None, 0, 0) == 0


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count if torch.cuda.is_available() else 256


def dry(lib, case):
    s = (C.c_int64 * len(case.sizes))(*case.sizes)
    f = (C.c_float * len(case.scalars))(*case.scalars)
    # 16-byte aligned addresses that are never read; a thin case whose D sits off its alignment keeps that
    p = (C.c_void_p * len(case.bufs))(*[None if b is None else FAKE + 4 * b.off for b in case.bufs])
    rc = lib.snerf_train_kernel_debug(case.op.encode(), s, len(case.sizes), f, len(case.scalars), p, len(case.bufs), None)
    assert rc >= 0, (case.id, lib.snerf_last_error())
    return rc


def test_every_case_dry_runs_to_what_it_names(lib):
    seen, reductions, split = set(), set(), 0
    for case in CASES + BIG:
        rc = dry(lib, case)
        if case.op != "wgrad":
            assert rc == wc.THIN_KERNELS[case.kernel], case.id
            seen.add(rc)
            continue
        got = wc.unpack(rc)
        assert [(g.kernel, g.partial) for g in got] == wc.expected_launches(case.par, _cus()), (case.id, got)
        assert all(g.reverse == 0 for g in got) or case.par["M"] >= 32768
        seen |= {g.kernel for g in got}
        reductions |= {(g.kernel, g.partial) for g in got}
        split += len(got) == 2
    assert seen == set(wc.WGRAD_KERNELS.values()) | set(wc.THIN_KERNELS.values())
    if _cus() == 256:
        # both reductions on every block shape, with and without the ride (FULL runs on atomics below eight row blocks like the others)
        assert reductions == {(k, p) for k in wc.WGRAD_KERNELS.values() for p in (0, 1)}, sorted(reductions)
        for c in CASES:                                      # 897 rows: eight row blocks - partial sums where the coverage rule allows, atomics for the thin blocks
            if c.op == "wgrad" and c.par["M"] == 897 and len(c.par["inst"]) == 1:
                assert wc.plan(897, c.par["n_out"], c.par["n_in"])[2][0] == 8
        thin_blocks = {(c.par["n_out"], c.par["n_in"]) for c in CASES if c.op == "wgrad" and c.par["M"] == 897 and not wc.expected_launches(c.par)[0][1]}
        assert thin_blocks == {(64, 64), (37, 100), (12, 128), (200, 63)}
    assert split >= 18


def test_a_dry_run_takes_no_turn(lib):
    big = next(c for c in BIG if c.par["bn"] == 0)
    d = {wc.unpack(dry(lib, big))[0].reverse for _ in range(5)}
    assert len(d) == 1                                       # five plans for inspection, one direction: the next launch's, left to it


def engine_layers(W, n_classes=4):
    """(name, n_out, n_in, bn) of every layer, from build_layers of csrc/train.cpp"""
    src = open(os.path.join(REPO, "season_nerf_amd", "csrc", "train.cpp")).read()
    body = src[src.index("static void build_layers("):]
    body = body[:body.index("\n}\n")]
    env = {"W": W, "C": n_classes, "W2": W // 2, "W4": W // 4}
    assert re.search(r"W2 = layer_width / 2; t->W4 = layer_width / 4;", src)
    out = []
    for m in re.finditer(r'add\("([\w.]+)",\s*([^,]+),\s*([^,]+),\s*(true|false),\s*(true|false)\);', body):
        out.append((m.group(1), int(eval(m.group(2), {}, env)), int(eval(m.group(3), {}, env)), m.group(5) == "true"))
    assert len(out) == 27 and out[4][0].endswith("fc5")
    return out


def test_the_engines_weight_gradients_land_on_covered_instances(lib):
    covered = set()
    for case in CASES + BIG:
        if case.op == "wgrad":
            covered |= {(g.kernel, g.partial) for g in wc.unpack(dry(lib, case))}
    n = 0
    for W in (64, 256, 512):
        for name, n_out, n_in, bn in engine_layers(W):
            for M in (33 * 37, 4096 * 10, 4096 * 96):       # a test's step, and per-point batches of the benchmark's size
                if n_out <= 4 and M >= 1024:
                    continue                                 # a thin head: the stream (route_wgrad)
                for ride in ((0, 1) if bn else (0,)):        # (the ride needs the dgrad below to have applied the activation backward: both forms occur)
                    for tab_cols in {0, n_in, W if n_in > W else n_in}:      # the input: materialised, stored as pre-activations, or [pre-activations | encoding]
                        case = wc.Case("engine", "wgrad", [M, n_out, n_in, n_out, n_in + 1, n_in, tab_cols, n_out if ride else 0, M if ride else 0, 1], [30.0, 30.0],
                                       [wc.Buf(k, None, None, "in") if on else None for k, on in
                                        [("dZ", 1), ("In", 1), ("dW", 1), ("tab", tab_cols)] + [(k, ride) for k in ("z", "gamma", "mu", "istd", "sdy", "sdyx", "dbias")]],
                                       "wgrad", None, None)
                        got = wc.unpack(dry(lib, case))
                        assert len(got) == (2 if ride and n_in > 256 else 1), (W, name, got)
                        assert {(g.kernel, g.partial) for g in got} <= covered, (W, name, M, got)
                        n += 1
    assert n > 300
