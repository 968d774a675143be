"""The weight gradients of the training engine, one kernel instance at a time through snerf_train_kernel_debug ("wgrad": run_wgrad on the Rows route,
its two-launch split included; "thin_wgrad" / "thin_fwd": the thin heads' streams with their second address), against the float64 references of
tests/wgrad_cases.py - the ten instances of wgrad_bf16x3_kernel<FULL, BNZ, TA, TB>, both reductions, both stage orders, the BatchNorm ride.

Per case (buffers as in tests/test_gpu_train_kernels.py, whose DeviceBuf this file uses): every matrix with ld > C - no two leading dimensions of a
case alike - and two extra rows behind it; NaN in the padding and tail rows of the inputs; a sentinel in the padding of dZ (under the ride), dW and
dbias that must come back bit for bit, the rows of dZ past M included; dW and dbias start from non-zero contents; without the ride dZ is an input and
must come back bit for bit as a whole.  The hook's return value must name the instance(s) and the reduction the case was built for
(wgrad_cases.expected_launches, with this device's CU count) and direction 0 below 32768 rows.  Every call is made twice into fresh buffers.  At
32768 + 77 rows one case per block shape is launched four times: both directions must occur, every launch meets the tolerance, and on the
partial-sum route two launches of one direction give the same bits of dW.  For every shape that can carry the ride, the ride agrees with
bn_bwd2_kernel / colpass_vec_kernel<4> followed by the plain weight gradient (dZ within its tolerance, dW within twice its own).

Tolerance: FACTOR * (E + 2^-24 * scale), FACTOR = 4 for every output (wgrad_cases.bounds: E measured on the CPU per case - for dW of the MFMA kernel
the fp32 evaluation's deviation plus the three-term split product's; dbias was examined for a wider margin and needs none).  NaN passes nowhere.

Measured on an MI355X (436 cases twice, 5 cases of 32845 rows four times, 16 ride comparisons; no kernel failed, none was changed) - per kernel the
largest E over its cases and the worst deviation as a fraction of the tolerance, per output (the large E figures belong to sums of 32845 terms at
alpha = 30; dW sits at a quarter of its tolerance everywhere because the kernel's error IS the split product's, which E contains):
    kernel                       E(dW)     dW      dZ      dbias  E(dbias)      kernel                      E         worst
    wgrad<F,F,1,2>               1.8e-04   0.249   -       -      -             thin_wgrad_kernel<false>    3.3e-05   0.179 (dW)  0.170 (dW3)
    wgrad<F,T,1,2>               2.0e-01   0.245   0.209   0.475  3.8e-02       thin_wgrad_kernel<true>     6.1e-05   0.196 (dW)  0.157 (dW3)
    wgrad<F,F,2,2>               3.6e-02   0.248   -       -      -             thin_fwd_kernel<false>      2.2e-06   0.154
    wgrad<F,T,2,2>               3.2e-02   0.251   0.194   0.358  3.8e-03       thin_fwd_kernel<true>       2.0e-06   0.145
    wgrad<F,F,1,4>               1.7e-04   0.247   -       -      -
    wgrad<F,T,1,4>               2.3e-01   0.245   0.195   0.383  4.1e-02
    wgrad<F,F,2,4>               3.7e-02   0.243   -       -      -
    wgrad<F,T,2,4>               2.9e-02   0.244   0.202   0.267  3.3e-03
    wgrad<T,F,2,4>               3.3e-02   0.244   -       -      -
    wgrad<T,T,2,4>               2.3e-01   0.246   0.207   0.452  7.0e-02
(E of dZ: 5e-07 .. 8e-07.  dbias in the kernel's order of additions, emulated on the CPU: at most 0.47 of the tolerance, tests/test_wgrad_refs.py.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import wgrad_cases as wc
from test_gpu_train_kernels import DeviceBuf, call_hook

pytestmark = pytest.mark.gpu

RETURNED = {}            # case id -> the launches the hook reported (wgrad) / the kernel number (thin)
FIGURES = {}             # "kernel output" -> [largest E, worst deviation / tolerance]


@pytest.fixture(scope="module")
def L():
    import season_nerf_amd as sn
    return sn._lib.lib()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def check_outputs(case, outs, rep):
    """every output of the case against float64"""
    want = wc.bounds(case)
    names = case.kernel if case.op == "wgrad" else (case.kernel,)
    for name, (val, tol, e, _) in want.items():
        got = outs[name].astype(np.float64).reshape(val.shape)
        err = np.abs(got - val)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = float(np.max(np.where(err == 0, 0.0, err / tol))) if err.size else 0.0
        print(f"FIG {'+'.join(names)} {case.id} {name} E={e:.3e} worst={ratio:.3f}")
        for k in (names if name == "dW" or case.op != "wgrad" else names[:1]):          # (dZ and dbias are the first launch's: the one with the ride)
            fig = FIGURES.setdefault(f"{k} {name}", [0.0, 0.0])
            fig[0], fig[1] = max(fig[0], e), max(fig[1], ratio if np.isfinite(ratio) else np.inf)
        ok = err <= tol                               # (NaN compares false)
        assert ok.all(), f"{case.id} launch {rep} {name}: {int((~ok).sum())} of {ok.size} outside FACTOR * (E + 2^-24 scale); worst {ratio:.2f} x the tolerance, E {e:.3e}"
    for b in case.bufs:
        if b is not None and b.role != "in":
            assert b.name in want, f"{case.id}: output {b.name} has no reference"


def launch(L, case):
    """one call into fresh buffers -> (what the hook returned, {buffer name: its data region afterwards}); DeviceBuf.read asserts that every byte outside
    an output's region - and every byte of an input - is what it was"""
    bufs = [DeviceBuf(b) if b is not None else None for b in case.bufs]
    rc = call_hook(L, case, bufs)
    return rc, {d.b.name: d.read() for d in bufs if d is not None}


def check_choice(case, rc):
    if case.op != "wgrad":
        assert rc == wc.THIN_KERNELS[case.kernel], f"{case.id}: the launcher chose kernel {rc}, the case was built for {case.kernel}"
        return rc
    got = wc.unpack(rc)
    assert [(g.kernel, g.partial) for g in got] == wc.expected_launches(case.par, _cus()), \
        f"{case.id}: launched {[(wc.KERNEL_NAMES.get(g.kernel), g.partial) for g in got]}, built for {case.kernel}"
    return got


def run_case(L, case):
    for rep in range(2):                                  # twice, into fresh buffers
        rc, outs = launch(L, case)
        RETURNED[case.id] = check_choice(case, rc)
        if case.op == "wgrad":
            assert all(g.reverse == 0 for g in RETURNED[case.id]), f"{case.id}: a launch below 32768 rows took a direction"
        check_outputs(case, outs, rep)


@pytest.mark.parametrize("case", wc.all_cases(), ids=lambda c: c.id)
def test_kernel_against_float64(L, case):
    run_case(L, case)


@pytest.mark.parametrize("case", wc.big_cases(), ids=lambda c: c.id)
def test_both_stage_orders(L, case):
    """32768 + 77 rows, four launches in a row: the direction alternates per launch (the process-wide turn), each launch meets the tolerance on dW, dbias
    and dZ, and on the partial-sum route two launches of one direction agree bit for bit on dW (a fixed order of additions)"""
    seen = {}
    for rep in range(4):
        rc, outs = launch(L, case)
        got = check_choice(case, rc)
        RETURNED[f"{case.id}#{rep}"] = got
        check_outputs(case, outs, rep)
        d = got[0].reverse
        if d in seen and got[0].partial:
            assert np.array_equal(seen[d].view(np.uint32), outs["dW"].view(np.uint32)), f"{case.id}: two launches of direction {d} differ in dW"
        seen.setdefault(d, outs["dW"])
    assert set(seen) == {0, 1}, f"{case.id}: four launches took the directions {sorted(seen)}"
    assert got[0].partial == 1


RIDE_SHAPES = [c for c in wc.all_cases() if c.op == "wgrad" and c.par["bn"] and c.par["M"] == 897 and c.par["tab_cols"] in (0, 256, 512)
               and (len(c.par["inst"]) == 2 or c.par["tab_cols"] == 0)]


@pytest.mark.parametrize("case", RIDE_SHAPES, ids=lambda c: c.id)
def test_ride_agrees_with_the_separate_pass(L, case):
    """the ride against the two kernels it replaces, in this process: bn_bwd2 (d_is_dy) on the same dY, then the plain weight gradient on its dZ"""
    _, ride = launch(L, case)
    par = case.par
    bufs = {b.name: DeviceBuf(b) for b in case.bufs if b is not None}
    n_out = par["n_out"]
    beta = DeviceBuf(wc.Buf("beta", np.zeros(n_out, np.float32), None, "in"))
    two = wc.Case(case.id + "-bn_bwd2", "bn_bwd2", [par["M"], n_out, bufs["z"].ld, bufs["dZ"].ld, par["M_global"], 1], [par["bias_alpha"]], None, None, None, None)
    rc = call_hook(L, two, [bufs[k] if k != "beta" else beta for k in ("z", "dZ", "mu", "istd", "gamma", "beta", "sdy", "sdyx", "dbias")])
    assert rc in (7, 6), rc                                   # bn_bwd2_kernel or colpass_vec_kernel<4>
    plain = case._replace(sizes=case.sizes[:7] + [0, 0, 1], bufs=list(case.bufs[:4]) + [None] * 7)
    rc = call_hook(L, plain, [bufs[k] if k in bufs else None for k in ("dZ", "In", "dW", "tab")] + [None] * 7)
    assert all(g.kernel % 2 == 0 for g in wc.unpack(rc))     # the instances without BNZ
    want = wc.bounds(case)
    for name, factor in (("dZ", 1.0), ("dW", 2.0), ("dbias", 2.0)):
        a, b = ride[name].astype(np.float64), bufs[name].read().astype(np.float64)
        ok = np.abs(a - b) <= factor * want[name][1]
        assert ok.all(), f"{case.id} {name}: ride and separate pass differ by {float(np.max(np.abs(a - b) / want[name][1])):.2f} x the tolerance"


def test_every_instance_reduction_and_direction_is_reached(L):
    """the launches the hook reported over the case list: all ten instances, each with both reductions, both directions, one launch and two; and the four
    variants of the thin streams (cases not run yet in this process are run here)"""
    for case in wc.all_cases():
        if case.id not in RETURNED:
            run_case(L, case)
    for case in wc.big_cases():
        if f"{case.id}#3" not in RETURNED:
            test_both_stage_orders(L, case)
    launches = [g for v in RETURNED.values() if isinstance(v, list) for g in v]
    assert {g.kernel for g in launches} == set(wc.WGRAD_KERNELS.values()), sorted(set(wc.WGRAD_KERNELS.values()) - {g.kernel for g in launches})
    if _cus() == 256:
        assert {(g.kernel, g.partial) for g in launches} == {(k, p) for k in wc.WGRAD_KERNELS.values() for p in (0, 1)}
    assert {g.partial for g in launches} == {0, 1} and {g.reverse for g in launches} == {0, 1}
    assert {(g.reverse, g.kernel % 2) for g in launches} == {(0, 0), (0, 1), (1, 0), (1, 1)}          # both directions with and without the ride
    assert {len(v) for v in RETURNED.values() if isinstance(v, list)} == {1, 2}
    assert {v for v in RETURNED.values() if not isinstance(v, list)} == set(wc.THIN_KERNELS.values())
    for k, (e, w) in sorted(FIGURES.items()):
        print(f"SUMMARY {k}: largest E {e:.3e}, worst deviation / tolerance {w:.3f}")
