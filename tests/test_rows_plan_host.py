"""The routing of the bf16x3 row GEMMs (csrc/gemm.hip plan_gemm_rows) pinned on the host: dry runs through snerf_rows_debug_set need no GPU (the CU
count falls back to 256).  Three things:
  * the table of kernel instances the three dispatchers can launch (run_gemm_rows / launch_gemm_rows16 / launch_gemm_areg), stated here a second time;
  * every case of tests/rows_cases.py dry-runs to the instance it names;
  * a bounded sweep of shapes x options x switch settings: every plan names an instance of the table with the divisibility its kernel needs, and the
    instances the sweep reaches are exactly the ones the case list covers - the rest of the table is UNREACHABLE, with the condition that excludes it."""
import ctypes as C
import os

import pytest

import rows_cases as rc
from rows_cases import AREG, FULL, GENERAL, ROWS16, Inst

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hooks():
    import importlib.util
    spec = importlib.util.spec_from_file_location("snerf_build", os.path.join(REPO, "season_nerf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()                      # no-op when the .so is up to date
    import season_nerf_amd as sn
    h = rc.Hooks(sn._lib.lib())
    yield h
    h.clear()


def dispatch_table():
    """The instances that exist, read off the dispatch functions (not off plan_gemm_rows)."""
    t = set()
    forms = ((0, 0), (1, 0), (0, 1))                                   # (AOL, ACT): plain, activation on load, activation backward
    for nt in (1, 2, 4):                                               # run_gemm_rows -> launch_full_nt<NT> -> launch_full<NT, PF>
        for pf in (2, 4, 8):
            t |= {Inst(FULL, nt, pf, aol, act, 1) for aol, act in forms if not (nt == 1 and act)}
    for nt in (2, 4):                                                  # run_gemm_rows -> launch_general<NT>
        t |= {Inst(GENERAL, nt, 0, aol, act, 1) for aol, act in forms}
    for nt in (4, 8):                                                  # launch_gemm_rows16 -> launch_rows16_nt<NT> -> launch_rows16<NT, PF>
        for pf in (1, 2, 4):
            t |= {Inst(ROWS16, nt, pf, aol, act, 1) for aol, act in (forms if pf < 4 else ((1, 0),)) if not (nt == 4 and act)}
    for aol in (0, 1):                                                 # launch_gemm_areg
        t.add(Inst(AREG, 8, 4, aol, 0, 2))
    for nt in (8, 16):
        for pf in (4, 8):
            t |= {Inst(AREG, nt, pf, aol, act, 1) for aol, act in forms}
    return t


TABLE = dispatch_table()

# instances of the table no shape and no switch setting leads to, and why.  (Removing these instantiations is a later change.)
UNREACHABLE = {
    Inst(FULL, 2, 8, 0, 1, 1): "plan_gemm_rows caps PF at 4 for the activation-backward epilogue (it needs the registers); SNERF_GEMM_PF can only lower PF",
    Inst(FULL, 4, 8, 0, 1, 1): "as above",
}


def test_instance_table():
    assert len(TABLE) == 24 + 6 + 12 + 14
    assert set(UNREACHABLE) <= TABLE
    assert set(rc.COVERED) <= TABLE
    assert not set(rc.COVERED) & set(UNREACHABLE)


def test_hooks_default_state_and_errors(hooks):
    L = hooks.L
    hooks.clear()
    assert hooks.read() == []
    bad = (C.c_int * 8)(1, 1, 2, 1, 3, 1, 1, 1)
    assert L.snerf_rows_debug_set(bad, 0, 0) == -1 and b"pf" in L.snerf_last_error()
    assert L.snerf_rows_record_read(None, 4) == -1
    # a dry run records thin-head and exact-fp32 routes as such, and checks arguments as a launch does
    a = rc.FAKE
    hooks.set((), dry_run=True)
    hooks.reset(False)
    assert L.snerf_linear_forward(5000, 128, 3, a, 128, a, a, 1.0, a, 4, None, 1, a, 1 << 20, None, 0, None) == 0           # thin head: a stream
    assert L.snerf_linear_forward(5000, 128, 64, a, 128, a, a, 1.0, a, 64, None, 0, None, 0, None, 0, None) == 0             # precision 0
    assert L.snerf_linear_dgrad(777, 64, 640, a, 640, a, 64, 1.0, 0, a, 64, 1, a, 1 << 22, None, 0, None, None, None, None, None) == 0      # 40 k-steps: no LDS-resident layout
    assert L.snerf_linear_forward(5000, 128, 64, a, 128, a, a, 1.0, a, 64, None, 1, None, 0, None, 0, None) == -1            # no scratch
    assert L.snerf_linear_forward(0, 128, 64, None, 128, None, None, 1.0, None, 64, None, 1, None, 0, None, 0, None) == 0    # empty batch: nothing routed
    got = hooks.read()
    assert sorted(p.route for p in got) == [rc.ROUTE_THIN, rc.ROUTE_FP32] and all(p.kernel == -1 for p in got)
    hooks.clear()
    assert hooks.read() == []


def test_every_case_dry_runs_to_its_instance(hooks):
    assert len(rc.CASES) == len(set(rc.CASES))
    per = {}
    for c in rc.CASES:
        M = rc.case_rows(hooks, c)
        p = rc.dry_plan(hooks, c, M)
        assert p is not None and p.route == rc.ROUTE_ROWS, c
        assert rc.plan_inst(p) == c.inst, (c, p)
        assert p.zero_bn == int(c.epi == "plain" and p.kernel in (FULL, ROWS16)), (c, p)
        if c.rows == "ragged":                 # more tiles than workers, fewer than two per worker, the last one ragged
            t, w = rc.tile_rows(c.inst), rc.n_workers(c.inst, p.grid, c.N)
            assert w >= 8 and w * t < M < 2 * w * t and M % t, (c, p)
        per.setdefault(c.inst, []).append(c)
    for inst, cs in per.items():               # what the issue asks of every covered instance
        base = [c for c in cs if not (c.pad_a or c.pad_c or c.a_off or c.x_padded or c.accumulate or c.epi == "plain" or c.K % 16)]
        assert {c.rows for c in base} >= set(rc.ROW_KINDS), inst
        assert len({rc.ksteps(c.K) for c in base}) >= 2, inst
        assert any(c.pad_a and c.pad_c for c in cs), inst
        if inst.aol:
            assert any(c.act_cols == c.K for c in cs) and any(0 < c.act_cols < c.K and not c.x_padded and c.K % 16 == 0 for c in cs), inst
        if inst.act:
            assert {c.epi for c in cs} == {"bn", "plain"}, inst
    assert any(c.accumulate and c.inst.act for c in rc.CASES) and any(c.accumulate and not c.inst.act for c in rc.CASES)
    print(f"{len(rc.CASES)} cases on {len(per)} instances")


SETTINGS = [(), (("areg", 0),), (("areg", 2),), (("areg_act", 0),), (("areg_hv", 1),), (("full", 0),), (("pf", 2),), (("pf", 4),), (("pf", 8),), (("gemm16", 0),),
            (("gemm16_k320", 0),), (("snake", 0),), (("areg", 0), ("gemm16", 0)), (("areg", 0), ("full", 0))]
N_TILES = (1, 2, 3, 4, 6, 8, 16)        # (pruned from 1..16: counts the kernels' group sizes 1, 2, 4 divide or do not, both widths of the AGPR kernel)


def _sweep_shapes():
    """(op, M, K, N, a_off, lda, act_cols, stats, epi, accumulate, x_padded) - forward and dgrad"""
    for ks in range(1, 39):
        for K, xp in ((16 * ks, False), (16 * ks - 1, True), (16 * ks - 7, False)):
            for nt in N_TILES:
                for N in (32 * nt, 32 * nt - 5):
                    lda0 = 16 * ks if xp else K
                    for a_off, lda, M in ((0, lda0, 1000), (1, lda0, 1000), (0, lda0 + 1, 1000), (0, lda0 + 4, (1 << 29) // N + 1)):
                        if (a_off or lda % 4 or M > 1000) and nt not in (1, 4, 8, 16):          # (the refused alignments and the offset limit: on four widths)
                            continue
                        for ac in sorted({0, K // 32 * 32, K // 16 * 16, 16 if K > 16 else 0, 8 if K > 8 else 0}):
                            yield ("fwd", M, K, N, a_off, lda, ac, ac == 0, None, False, xp)
                        if not xp:
                            for epi in (None, "bn", "plain"):
                                for acc in (False, True):
                                    yield ("dgrad", M, K, N, a_off, lda, 0, False, epi, acc, False)


def _check_plan(p, shape):
    op, M, K, N, a_off, lda, ac, stats, epi, acc, xp = shape
    ks, n_tiles = rc.ksteps(K), (N + 31) // 32
    inst = rc.plan_inst(p)
    assert p.route == rc.ROUTE_ROWS and inst in TABLE, (shape, p)
    assert inst.aol == int(ac > 0) and inst.act == int(epi is not None), (shape, p)
    assert p.grid >= 1 and 0 < p.lds <= rc.LDS_MAX, (shape, p)
    if inst.kernel == FULL:
        assert n_tiles % inst.nt == 0 and (inst.nt > 1 or n_tiles == 1) and ks % inst.pf == 0 and p.lds >= inst.nt * ks * 2048 + 8 * ac, (shape, p)
        assert (N == 32 * n_tiles or inst.nt == 1) and not acc and a_off == 0 and lda % 4 == 0 and M * N < 1 << 29 and (K % 16 == 0 or xp), (shape, p)
    elif inst.kernel == ROWS16:
        assert (2 * n_tiles) % inst.nt == 0 and N == 32 * n_tiles and ks % 2 == 0 and (ks // 2) % inst.pf == 0, (shape, p)
        assert p.lds >= inst.nt * (ks // 2) * 2048 + 8 * ac and not acc and a_off == 0 and lda % 4 == 0 and M * N < 1 << 29 and (K % 32 == 0 or xp) and ac % 32 == 0, (shape, p)
    elif inst.kernel == AREG:
        assert N in (256, 512) and ks % inst.pf == 0 and 8 <= ks <= 64 and ks % 4 == 0, (shape, p)
        assert (inst.nt, inst.pf) == (8, 4) and N == 512 if inst.hv == 2 else inst.nt * 32 == N, (shape, p)
        assert not acc and a_off == 0 and lda % 4 == 0 and M * N < 1 << 29 and (K % 16 == 0 or xp) and ac % 16 == 0, (shape, p)
    else:
        assert inst.pf == 0 and p.lds >= inst.nt * ks * 2048, (shape, p)


def test_sweep_names_instances_and_matches_the_case_list(hooks):
    L = hooks.L
    shapes = list(_sweep_shapes())
    reached = {}
    a = rc.FAKE
    sb = 1 << 26
    buf = hooks.buf
    n = 0
    for sw in SETTINGS:
        for xp in (False, True):
            hooks.set(sw, dry_run=True, x_padded=xp)
            for s in shapes:
                op, M, K, N, a_off, lda, ac, stats, epi, acc, sxp = s
                if sxp != xp:
                    continue
                L.snerf_rows_record_reset(0)
                if op == "fwd":
                    r = L.snerf_linear_forward(M, K, N, a + 4 * a_off, lda, a, a, 30.0, a, N, a if stats else None, 1, a, sb, a if ac else None, ac, None)
                else:
                    e = a if epi else None
                    b = a if epi == "bn" else None
                    r = L.snerf_linear_dgrad(M, N, K, a + 4 * a_off, lda, a, N, 30.0, int(acc), a, N, 1, a, sb, e, N, e, b, b, e, None)
                assert r == 0, (sw, s, L.snerf_last_error())          # every shape of the sweep has a plan: no setting makes a product an error
                assert L.snerf_rows_record_read(buf, 2) == 1, (sw, s)
                p = rc.Plan(*buf[0:12])
                _check_plan(p, s)
                reached.setdefault(rc.plan_inst(p), (sw, s))
                n += 1
    hooks.clear()
    print(f"{n} plans, {len(reached)} instances reached")
    never = TABLE - set(reached)
    assert never == set(UNREACHABLE), (sorted(never - set(UNREACHABLE)), sorted(set(UNREACHABLE) - never))
    missing = set(reached) - set(rc.COVERED)
    assert not missing, {rc.inst_name(i): reached[i] for i in missing}
    assert set(rc.COVERED) == set(reached)
