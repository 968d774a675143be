"""Every kernel instance the bf16x3 row GEMMs can be routed to (csrc/gemm.hip plan_gemm_rows -> gemm_rows_full_kernel, gemm_rows_kernel,
gemm_rows16_kernel, gemm_areg_kernel), launched on purpose - the case list of tests/rows_cases.py, one test per instance - and compared with a float64
matmul of the same operands.  Per case: the plan record (snerf_rows_record_*) must hold exactly the instance the case names; sentinels sit in the
padding columns and in the rows past M of the output, NaNs in the padding columns of the input; the column sums are checked where the call has them.
Tolerances are those of tests/test_gpu_linear.py.  The equalities the sources claim between the kernels are checked in-process through the switch
override (snerf_rows_debug_set), and one training step per width must run on covered instances only."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rows_cases as rc
from rows_cases import AREG, FULL, GENERAL, ROWS16
from test_gpu_linear import TOL

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23


@pytest.fixture()
def env():
    import season_nerf_amd as sn
    L = sn._lib.lib()
    h = rc.Hooks(L)
    h.clear()
    yield SimpleNamespace(sn=sn, L=L, hooks=h, st=C.c_void_p(torch.cuda.current_stream().cuda_stream))
    h.clear()


class Operands:
    """Inputs of a case at M rows and its float64 reference."""

    def __init__(self, L, case, M, seed):
        c = case
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        rnd = lambda *s: torch.randn(*s, device="cuda", generator=g)
        uni = lambda *s: torch.rand(*s, device="cuda", generator=g)
        K, N, lda, ldc = c.K, c.N, rc.lda_of(c), rc.ldc_of(c)
        self.case, self.M, self.ldc = c, M, ldc
        flat = torch.empty(M * lda + 8, device="cuda")
        A = flat[c.a_off:c.a_off + M * lda].view(M, lda)
        A.copy_(rnd(M, lda) * (4 if c.act_cols else 1))                       # (activation on load: SIREN-sized pre-activations)
        kz = rc.ksteps(K) * 16 if c.x_padded else K
        A[:, K:kz] = 0.0                                                      # the zero padding the caller promises
        A[:, kz:] = float("nan")                                              # columns no kernel may read
        self.A_keep, self.A = flat, A
        self.W = rnd(N, K) / K ** 0.5 if c.op == "fwd" else rnd(K, N) / K ** 0.5      # [n_out, n_in]
        self.bias = rnd(N)
        self.scratch = torch.empty(L.snerf_linear_scratch_bytes(K, N), dtype=torch.uint8, device="cuda")
        self.base = rnd(M, N) if c.accumulate else None
        Ad = A[:, :K].double()
        if c.op == "fwd":
            ac = c.act_cols
            if ac:
                mu, istd, gam, bet = rnd(ac).double(), (uni(ac) + 0.5).double(), (uni(ac) + 0.5).double(), rnd(ac).double()
                self.tab = torch.stack([gam * istd / (2 * np.pi), (bet - gam * mu * istd) / (2 * np.pi)]).float().contiguous()
                Ad = Ad.clone()
                Ad[:, :ac] = torch.sin(gam * ((Ad[:, :ac] - mu) * istd) + bet)
            self.prod = 30.0 * (Ad @ self.W.double().T)                       # without the bias: what the BatchNorm sums are taken of
            self.ref = self.prod + 30.0 * self.bias.double()
            self.ref0 = self.prod
        else:
            self.ref = 30.0 * (Ad @ self.W.double()) + (self.base.double() if c.accumulate else 0.0)
            if c.epi:
                self.z = rnd(M, N + 4) * 4
                bn = c.epi == "bn"
                mu, istd = (rnd(N).double(), (uni(N) + 0.5).double()) if bn else (torch.zeros(N, device="cuda").double(), torch.ones(N, device="cuda").double())
                gam, bet = ((uni(N) + 0.5).double(), rnd(N).double()) if bn else (torch.ones(N, device="cuda").double(), torch.zeros(N, device="cuda").double())
                self.etab = torch.stack([gam * istd / (2 * np.pi), (bet - gam * mu * istd) / (2 * np.pi)]).float().contiguous()
                self.mu, self.istd = mu.float(), istd.float()
                self.xh = (self.z[:, :N].double() - mu) * istd
                self.ref = self.ref * torch.cos(gam * self.xh + bet)

    def launch(self, env, sw, expect, bias=True):
        """One launch under the switches `sw`; asserts the record holds exactly one plan, of an instance in `expect`.  Returns (output buffer, sums, plan)."""
        c, M, L = self.case, self.M, env.L
        out = torch.full((M + 3, self.ldc), 7.0, device="cuda")
        if c.accumulate:
            out[:M, :c.N] = self.base
        sums = torch.zeros(2, c.N, dtype=torch.float64, device="cuda")
        nul = torch.zeros(1, device="cuda")
        ptr = {"A": self.A_keep.data_ptr(), "W": self.W.data_ptr(), "bias": self.bias.data_ptr() if bias else None, "C": out.data_ptr(), "stats": sums.data_ptr(),
               "scratch": self.scratch.data_ptr(), "tab": getattr(self, "tab", nul).data_ptr(), "z": getattr(self, "z", nul).data_ptr(),
               "etab": getattr(self, "etab", nul).data_ptr(), "mu": getattr(self, "mu", nul).data_ptr(), "istd": getattr(self, "istd", nul).data_ptr(), "sums": sums.data_ptr()}
        env.hooks.set(sw, x_padded=c.x_padded)
        env.hooks.reset(True)
        rcode = rc.call(L, c, M, ptr, env.st)
        got = env.hooks.read()
        env.hooks.clear()
        assert rcode == 0, (c, L.snerf_last_error())
        assert len(got) == 1 and got[0].route == rc.ROUTE_ROWS and rc.plan_inst(got[0]) in expect, (c, sw, got)
        return out, sums, got[0]

    def check(self, out, sums, bias=True):
        """Against float64: values, sentinels, column sums - the bounds of tests/test_gpu_linear.py."""
        c, M, N = self.case, self.M, self.case.N
        ref = self.ref if (bias or c.op != "fwd") else self.ref0
        tol = TOL[1] * (2 if (c.act_cols or c.epi) else 1)
        err = float((out[:M, :N].double() - ref).abs().max() / ref.abs().max())
        assert err < tol, (c, M, err)
        assert bool((out[:M, N:] == 7.0).all()) and bool((out[M:] == 7.0).all()), (c, M)          # padding columns and rows past M untouched
        s = sums.cpu().numpy()
        if c.op == "fwd" and c.stats:
            d = self.prod
            np.testing.assert_allclose(s[0], d.sum(0).cpu().numpy(), rtol=0, atol=2e-4 * float(d.abs().sum(0).max()), err_msg=str(c))
            np.testing.assert_allclose(s[1], (d * d).sum(0).cpu().numpy(), rtol=2e-4, atol=2e-4 * float((d * d).sum(0).max()), err_msg=str(c))
        if c.epi:
            np.testing.assert_allclose(s[0], ref.sum(0).cpu().numpy(), rtol=0, atol=3e-4 * float(ref.abs().sum(0).max()), err_msg=str(c))
            want = (ref * self.xh).sum(0).cpu().numpy() if c.epi == "bn" else np.zeros(N)
            np.testing.assert_allclose(s[1], want, rtol=0, atol=3e-4 * float((ref * self.xh).abs().sum(0).max()) + 1e-12, err_msg=str(c))
        return err


def _with(sw, **kw):
    return tuple(sorted(dict(dict(sw), **kw).items()))


GENERALS = {i for i in rc.COVERED if i.kernel == GENERAL}
COLUMN32 = {i for i in rc.COVERED if i.kernel in (GENERAL, FULL)}


def _equalities(env, ops, out, sums):
    """The equalities the sources claim between the kernels, on the inputs of the case.
    The column sums of two kernels are compared with the bounds of tools/compare_gemm_paths.py and tools/areg_check.py as they stand, on every case with more than
    one row.  Their absolute terms (1e-5 M, 2e-5 M) budget 1e-5 / 2e-5 of error per row, which holds where the rows' roundings average out.  At M = 1 a "sum" is one
    fp32 output d = v - alpha bias (as the column-group kernels form it) and its square: d alone carries up to 2^-23 |v| of rounding (|v| reaches ~100 here), and the
    16x16x32 form's outputs may differ by 4e-6 of the output scale by the same tool's bound - both above the per-row budget.  Measured at M = 1, alpha = 30: the AGPR
    kernel against gemm_rows_full_kernel up to 3.6e-5 absolute (8.9e-6 relative) on 1-3 of 512-1024 sums, the 16x16x32 form against gemm_rows_kernel up to 1.6e-4
    absolute (2.7e-4 relative on a sum of 0.13).  The one-row sums are still held to float64 by Operands.check, and the outputs to the bitwise / 4e-6 claims."""
    c, M = ops.case, ops.M
    k = c.inst.kernel
    if k == FULL:
        # gemm_rows_full_kernel: same fragments, same summation order as gemm_rows_kernel -> identical bits (csrc/gemm.hip; tools/compare_gemm_paths.py)
        o2, s2, _ = ops.launch(env, _with(c.sw, full=0), GENERALS)
        assert torch.equal(out, o2), (c, M)
        np.testing.assert_allclose(sums.cpu().numpy(), s2.cpu().numpy(), rtol=1e-6, atol=1e-5 * M, err_msg=str(c))
    elif k == ROWS16:
        # the 16x16x32 form sums the k terms of a 32-k step in another order: 4e-6 of the output scale, identical untouched cells (tools/compare_gemm_paths.py)
        o2, s2, _ = ops.launch(env, _with(c.sw, full=0), GENERALS)
        assert torch.equal(out == 7.0, o2 == 7.0), (c, M)
        scale = float(o2[o2 != 7.0].abs().max())
        assert float((out - o2).abs().max()) <= 4e-6 * scale, (c, M, float((out - o2).abs().max()) / scale)
        if M > 1:      # (see _equalities' docstring for the one-row cases)
            np.testing.assert_allclose(sums.cpu().numpy(), s2.cpu().numpy(), rtol=1e-5, atol=2e-5 * M, err_msg=str(c))
    elif k == AREG:
        # gemm_areg_kernel: same products, same k order, same order of the three partial products per accumulator as the 32x32x16 kernels
        # (csrc/gemm_areg.hip; tools/areg_check.py): the accumulators are the same bits.  Its forward epilogue folds the bias in as fma(alpha, acc, alpha * bias)
        # where the column-group kernels compute alpha * (acc + bias): without a bias (and in the activation-backward form, which has none) the outputs are
        # identical bits; with one, each side is within one rounding of alpha * bias and one of the result ("1 ulp").
        ref_sw = _with(c.sw, areg=0, gemm16=0)
        o2, s2, _ = ops.launch(env, ref_sw, COLUMN32)
        if c.op == "fwd":
            # |alpha (acc + bias)| (1 + u)^2 against |alpha bias| (1 + u) + ... (1 + u), u = 2^-24: at most 3 u |out| + u |alpha bias| apart
            bound = EPS32 * (30.0 * ops.bias.abs()[None, :] + 2.0 * out[:M, :c.N].abs())
            assert bool(((out[:M, :c.N] - o2[:M, :c.N]).abs() <= bound).all()), (c, M)
            a0, _, _ = ops.launch(env, c.sw, {c.inst}, bias=False)
            b0, _, _ = ops.launch(env, ref_sw, COLUMN32, bias=False)
            ops.check(a0, sums, bias=False)
            assert torch.equal(a0, b0), (c, M, float((a0 - b0).abs().max()))
        else:
            assert torch.equal(out, o2), (c, M, float((out - o2).abs().max()))
        if M > 1:
            np.testing.assert_allclose(sums.cpu().numpy(), s2.cpu().numpy(), rtol=2e-6, atol=1e-5 * M, err_msg=str(c))


@pytest.mark.parametrize("inst", rc.COVERED, ids=rc.inst_name)
def test_instance_against_float64(env, inst):
    worst = 0.0
    cases = rc.cases_of(inst)
    for i, c in enumerate(cases):
        M = rc.case_rows(env.hooks, c)
        ops = Operands(env.L, c, M, 1000 * rc.COVERED.index(inst) + i)
        out, sums, plan = ops.launch(env, c.sw, {inst})
        worst = max(worst, ops.check(out, sums))
        _equalities(env, ops, out, sums)
    print(f"  {rc.inst_name(inst)}: {len(cases)} cases, worst error {worst:.2e} of the output scale")


@pytest.mark.parametrize("inst", [i for i in rc.COVERED if i.kernel == ROWS16 and i.pf == 2], ids=rc.inst_name)
def test_rows16_tile_order_gives_identical_bits(env, inst):
    """gemm_rows16_kernel walks its row tiles forwards on one launch and backwards on the next once a launch has 32 768 rows (stream_direction,
    SNERF_SNAKE): with one 128- or 64-column group every CU is a worker, so the ragged row count of the case list is above that.  Two consecutive
    launches and one with SNERF_SNAKE=0 give the same bits, sums to double-atomic order."""
    base = [c for c in rc.cases_of(inst) if c.rows == "ragged"][0]
    c = base._replace(N=16 * inst.nt)
    M = rc.case_rows(env.hooks, c)
    assert M >= 32768
    ops = Operands(env.L, c, M, 77)
    outs = [ops.launch(env, sw, {inst}) for sw in (c.sw, c.sw, _with(c.sw, snake=0))]
    for o, s, _ in outs:
        ops.check(o, s)
        assert torch.equal(o, outs[0][0])


@pytest.mark.parametrize("W,classic", [(64, False), (64, True), (256, False), (512, False)])
def test_training_step_runs_on_covered_instances(env, W, classic):
    """Forward + backward of get_loss on 33 rays x 37 samples: every row-GEMM plan the engine executed is an instance the case list covers under the default switches."""
    from oracle import season_nerf_oracle as orc
    sn = env.sn
    Cn, R, S = 4, 33, 37
    net = sn.T_NeRF(W, Cn)
    net.load_state_dict(orc.init_weights(W, Cn, 9, bn_stats="identity"))
    net = net.to("cuda").train()
    rng = np.random.Generator(np.random.PCG64(12))
    T = lambda a: torch.tensor(a, dtype=torch.float32)
    sun = rng.uniform(0.1, 1, (R, 3)); sun /= np.linalg.norm(sun, axis=1, keepdims=True)
    tau = rng.uniform(0, 1, (R, 2))
    data = {"Top": T(np.concatenate([rng.uniform(-1, 1, (R, 2)), np.ones((R, 1))], 1)),
            "Bot": T(np.concatenate([rng.uniform(-1, 1, (R, 2)), -np.ones((R, 1))], 1)), "Sun_Angle": T(sun),
            "Time_Encoded": T(np.stack([np.cos(6.28 * tau[:, 0]), np.sin(6.28 * tau[:, 0]), np.cos(6.28 * tau[:, 1]), np.sin(6.28 * tau[:, 1])], 1)),
            "GT_Color": T(rng.uniform(0, 1, (R, 3)))}
    st = np.concatenate([rng.uniform(-1, 1, (R, 2)), np.ones((R, 1))], 1)
    solar = {"Top": T(st), "Bot": T(st - 2 * sun / sun[:, 2:]), "Sun_Angle": T(sun)}
    args = SimpleNamespace(n_samples=S, Use_Reg=True, Solar_Type_2=classic, Use_MSE_loss=True, Use_Solar=True, sc_lambda=0.03, number_low_frequency_cases=Cn)
    ev = sn.All_in_One_Eval(args, torch.device("cuda"), 10, False, None, np.eye(4), np.zeros(3))
    ev.solar_creation_tool = lambda n, include_times=True: (solar["Top"], solar["Bot"], solar["Sun_Angle"], torch.zeros(R, 4), None)
    env.hooks.reset(True)
    loss = ev.get_loss(data, net, 0, False)
    sum(v * w for v, w in loss.values()).backward()
    torch.cuda.synchronize()
    got = env.hooks.read()
    env.hooks.clear()
    ran = sorted({rc.plan_inst(p) for p in got if p.route == rc.ROUTE_ROWS})
    print(f"  W={W} Solar_Type_2={classic}: routes {sorted({p.route for p in got})}, row-GEMM instances:")
    for i in ran:
        print("    " + rc.inst_name(i))
    assert ran, "the engine ran no row GEMM"
    default = {c.inst for c in rc.CASES if c.sw == ()}
    assert set(ran) <= default, [rc.inst_name(i) for i in ran if i not in default]
