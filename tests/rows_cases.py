"""The case list of the row GEMMs' kernel instances, shared by tests/test_rows_plan_host.py (every case dry-runs to the instance it names) and
tests/test_gpu_rows_instances.py (every case runs on that instance and is compared with float64), and the few helpers both need: the switch
settings, the call of snerf_linear_forward / snerf_linear_dgrad from a case, the dry run, the block map of csrc/gemm_rows.h.

An instance is one separately compiled kernel: Inst(kernel, nt, pf, aol, act, hv) as the plan of csrc/gemm.hip plan_gemm_rows names it
(include/season_nerf_hip.h snerf_rows_record_read).  K is the reduction length (forward: n_in; dgrad: n_out), N the produced columns
(forward: n_out; dgrad: n_cols = n_in), `ks` counts 16-k steps of K.

How the values are chosen, per instance:
  k-step counts  the set of counts the instance can run at is written down (ALLOWED below, from the routing conditions); of it the smallest two -
                 PF and 2 PF wherever the set starts there; a column-group class that starts higher (NT = 2: 21..38 steps, the 64-column
                 16x16x32 form: 20..38) or gemm_areg_ok (at least 8 steps, a multiple of 4) moves them up - and the largest.  The 16x16x32
                 form counts 32-k steps.  Where the shape alone would pick a deeper pipeline, SNERF_GEMM_PF names the instance's.
  row counts     1, one tile - 1, one tile + 1, and n_workers * tile_rows + tile_rows / 2 + 3 (some workers take a second, ragged tile, others
                 none), n_workers from the plan's grid and the block map; tile_rows is 256 (column-group kernels) or 128 (AGPR kernel).
  variations     padded lda / ldc; activation on load over all of K (the base cases) and over a leading part; dgrad with the activation-backward
                 epilogue with (base) and without BatchNorm, and `accumulate` where the instance takes it; one zero-padded-K case (K = 63, 319
                 or 575) for every instance that can run at 4, 20 or 36 steps in a forward."""
import ctypes as C
from collections import namedtuple

AREG, ROWS16, FULL, GENERAL = 0, 1, 2, 3
KERNEL_NAMES = {AREG: "gemm_areg_kernel", ROWS16: "gemm_rows16_kernel", FULL: "gemm_rows_full_kernel", GENERAL: "gemm_rows_kernel"}
ROUTE_THIN, ROUTE_ROWS, ROUTE_FP32 = 0, 1, 2
Inst = namedtuple("Inst", "kernel nt pf aol act hv")
Plan = namedtuple("Plan", "route kernel nt pf aol act hv tab_lds zero_bn split grid lds")

SWITCH_NAMES = ("areg", "areg_act", "areg_hv", "full", "pf", "gemm16", "gemm16_k320", "snake")      # RowsSwitches, csrc/gemm_rows.h
SWITCH_DEFAULTS = dict(areg=1, areg_act=1, areg_hv=2, full=1, pf=0, gemm16=1, gemm16_k320=1, snake=1)
LDS_MAX = 160 * 1024


def inst_name(i):
    return f"{KERNEL_NAMES[i.kernel]}<nt={i.nt},pf={i.pf},aol={i.aol},act={i.act},hv={i.hv}>"


def plan_inst(p):
    return Inst(p.kernel, p.nt, p.pf, p.aol, p.act, p.hv)


def switch_values(over):
    d = dict(SWITCH_DEFAULTS, **dict(over))
    return tuple(d[n] for n in SWITCH_NAMES)


# op: "fwd" | "dgrad";  rows: "1" | "t-1" | "t+1" | "ragged" (or an int);  pad_a / pad_c: floats added to lda / ldc;  a_off: floats the A pointer is
# moved off its 16-byte alignment;  act_cols: activation on load (fwd);  stats: BatchNorm sums (fwd);  epi: None | "bn" | "plain" (dgrad's
# activation-backward epilogue);  sw: the switches moved off their defaults, as sorted (name, value) pairs
Case = namedtuple("Case", "inst op K N rows pad_a pad_c a_off act_cols stats epi accumulate x_padded sw")
ROW_KINDS = ("1", "t-1", "t+1", "ragged")


def tile_rows(inst):
    return 128 if inst.kernel == AREG else 256


def n_groups(inst, N):
    nt32 = (N + 31) // 32
    if inst.kernel == FULL:
        return nt32 // inst.nt
    if inst.kernel == GENERAL:
        return (nt32 + inst.nt - 1) // inst.nt
    return 2 * nt32 // inst.nt          # ROWS16: 16-column tiles


def n_workers(inst, grid, N):
    """SNERF_ROWS_BLOCK_MAP: block -> (XCD, slot), slots / n_groups whole workers per XCD; the AGPR kernel: one worker per workgroup."""
    if inst.kernel == AREG:
        return grid
    return ((grid >> 3) // n_groups(inst, N)) * 8


def rows_of(case, grid):
    t = tile_rows(case.inst)
    if isinstance(case.rows, int):
        return case.rows
    return {"1": 1, "t-1": t - 1, "t+1": t + 1, "ragged": n_workers(case.inst, grid, case.N) * t + t // 2 + 3}[case.rows]


def ksteps(K):
    return (K + 15) // 16


def lda_of(case):
    return (ksteps(case.K) * 16 if case.x_padded else case.K) + case.pad_a


def ldc_of(case):
    return case.N + case.pad_c


# ---------------------------------------------------------------------------------------------------------------------
# the library side: debug state, record, and the two public calls built from a case
class Hooks:
    def __init__(self, L):
        self.L = L
        self.buf = (C.c_int32 * (12 * 256))()

    def set(self, sw=(), dry_run=False, x_padded=False, own_switches=False):
        arr = None if own_switches else (C.c_int * 8)(*switch_values(sw))
        assert self.L.snerf_rows_debug_set(arr, int(dry_run), int(x_padded)) == 0, self.L.snerf_last_error()

    def clear(self):
        assert self.L.snerf_rows_debug_set(None, 0, 0) == 0
        assert self.L.snerf_rows_record_reset(0) == 0

    def reset(self, on=True):
        assert self.L.snerf_rows_record_reset(int(on)) == 0

    def read(self):
        n = self.L.snerf_rows_record_read(self.buf, 256)
        assert 0 <= n <= 256, n
        return [Plan(*self.buf[12 * i:12 * i + 12]) for i in range(n)]


FAKE = 1 << 24          # an aligned, non-null address: a dry run dereferences nothing


def call(L, case, M, ptr, stream=None):
    """snerf_linear_forward / snerf_linear_dgrad of a case.  ptr: name -> address for A, W, bias, C, stats, scratch, tab, z, etab, mu, istd, sums."""
    K, N = case.K, case.N
    sb = L.snerf_linear_scratch_bytes(K, N)
    if case.op == "fwd":
        return L.snerf_linear_forward(M, K, N, ptr["A"] + 4 * case.a_off, lda_of(case), ptr["W"], ptr["bias"], 30.0, ptr["C"], ldc_of(case),
                                      ptr["stats"] if case.stats else None, 1, ptr["scratch"], sb, ptr["tab"] if case.act_cols else None, case.act_cols, stream)
    epi = case.epi is not None
    return L.snerf_linear_dgrad(M, N, K, ptr["A"] + 4 * case.a_off, lda_of(case), ptr["W"], N, 30.0, int(case.accumulate), ptr["C"], ldc_of(case), 1,
                                ptr["scratch"], sb, ptr["z"] if epi else None, N + 4, ptr["etab"] if epi else None,
                                ptr["mu"] if case.epi == "bn" else None, ptr["istd"] if case.epi == "bn" else None, ptr["sums"] if epi else None, stream)


FAKE_PTRS = {k: FAKE for k in ("A", "W", "bias", "C", "stats", "scratch", "tab", "z", "etab", "mu", "istd", "sums")}


def dry_plan(hooks, case, M, sw=None):
    """The one record entry a dry run of the case at M rows leaves (None: the call was refused)."""
    hooks.set(case.sw if sw is None else sw, dry_run=True, x_padded=case.x_padded)
    hooks.reset(False)
    rc = call(hooks.L, case, M, FAKE_PTRS)
    got = hooks.read()
    hooks.set((), dry_run=False, x_padded=False, own_switches=True)
    if rc != 0:
        return None
    assert len(got) == 1, got
    return got[0]


def case_rows(hooks, case):
    """Rows of the case on this device: the grid comes from a dry run with more row tiles than the device has CUs."""
    p = dry_plan(hooks, case._replace(rows=100000), 100000)
    assert p is not None and p.route == ROUTE_ROWS, (case, p)
    return rows_of(case, p.grid)


# ---------------------------------------------------------------------------------------------------------------------
# the instance table as the case list sees it: for every instance the k-step counts it can run at (16-k steps), the N it is driven with and the
# switches that lead to it.  Read off plan_gemm_rows (csrc/gemm.hip); tests/test_rows_plan_host.py holds the table of the dispatchers and the sweep
# that checks both.
def _native_pf(ks, act):
    pf = 8 if ks % 8 == 0 else 4 if ks % 4 == 0 else 2 if ks % 2 == 0 else 0
    return min(pf, 4) if act else pf


def _pick(allowed):
    allowed = sorted(allowed)
    return sorted(set(allowed[:2] + allowed[-1:]))


def _sw(**kw):
    return tuple(sorted(kw.items()))


def _mk(inst, op, ks, N, sw, rows, **kw):
    d = dict(pad_a=0, pad_c=0, a_off=0, act_cols=0, stats=(op == "fwd"), epi=None, accumulate=False, x_padded=False, K=16 * ks)
    d.update(kw)
    if inst.aol and not d["act_cols"]:
        d["act_cols"] = d["K"] if not d["x_padded"] else d["K"] // 32 * 32
    if inst.act and d["epi"] is None:
        d["epi"] = "bn"
    return Case(inst=inst, op=op, N=N, rows=rows, sw=sw, **d)


def _family(inst, allowed, N, sw_for):
    """Base cases (k-step picks x row counts) and the variations of one instance.  sw_for(ks) -> switches that lead there."""
    op = "dgrad" if inst.act else "fwd"
    out = []
    picks = _pick(allowed)
    for ks in picks:
        for rows in ROW_KINDS:
            out.append(_mk(inst, op, ks, N, sw_for(ks), rows))
    ks = picks[1] if len(picks) > 1 else picks[0]
    out.append(_mk(inst, op, ks, N, sw_for(ks), "t+1", pad_a=4, pad_c=4))
    if inst.aol:
        unit = 32 if inst.kernel == ROWS16 else 16 if inst.kernel in (FULL, AREG) else 8
        lead = max(unit, (16 * picks[-1] // 2) // unit * unit)
        if lead < 16 * picks[-1]:
            out.append(_mk(inst, op, picks[-1], N, sw_for(picks[-1]), "t+1", act_cols=lead))
    if inst.act:
        out.append(_mk(inst, op, ks, N, sw_for(ks), "t+1", epi="plain"))
    if op == "fwd":
        for K in (63, 319, 575):
            if ksteps(K) in allowed:
                out.append(_mk(inst, op, ksteps(K), N, sw_for(ksteps(K)), "t+1", K=K, x_padded=True))
                break
    return out


def _build():
    cases = []
    # ---- gemm_rows_full_kernel<NT, PF, AOL, ACT>: NT = 1 thin heads (N <= 32, no ACT form); NT = 4 up to 20 k-steps (with a table: up to 19, at 20 the
    # LDS holds two n-tiles); NT = 2 for 22..38 (with a table: from 20).  By default the 16x16x32 form takes what it can of NT = 4 / 2: SNERF_GEMM16=0.
    for pf in (2, 4, 8):
        for aol, act in ((0, 0), (1, 0), (0, 1)):
            for nt in (1, 2, 4):
                if (nt == 1 and act) or (act and pf == 8):
                    continue
                lo, hi = {1: (1, 38), 4: (1, 19 if aol else 20), 2: (20 if aol else 21, 38)}[nt]
                allowed = [k for k in range(lo, hi + 1) if k % pf == 0]
                N = {1: 12, 4: 384, 2: 192}[nt]
                inst = Inst(FULL, nt, pf, aol, act, 1)

                def sw_for(ks, nt=nt, pf=pf, act=act):
                    kw = {} if nt == 1 else {"gemm16": 0}
                    if _native_pf(ks, act) != pf:
                        kw["pf"] = pf
                    return _sw(**kw)
                cases += _family(inst, allowed, N, sw_for)
    # ---- gemm_rows_kernel<NT, AOL, ACT>: NT = 4 up to 20 k-steps, 2 up to 38; whatever the full-tile forms refuse: here a ragged N (last group one tile short
    # and that tile 10 columns wide)
    for nt, (lo, hi), N in ((4, (1, 20), 330), (2, (21, 38), 170)):
        for aol, act in ((0, 0), (1, 0), (0, 1)):
            inst = Inst(GENERAL, nt, 0, aol, act, 1)
            allowed = [k for k in range(lo, hi + 1) if k % 4 == 0] + [lo, hi]          # its fixed four k-steps of A in flight: 4, 8 where the class has them
            fam = _family(inst, allowed, N, lambda ks: ())
            op = "dgrad" if act else "fwd"
            ks = sorted(set(allowed))[1]
            fam.append(_mk(inst, op, ks, N, (), "t+1", a_off=1, pad_a=1))              # unaligned rows: scalar loads
            fam.append(_mk(inst, op, ks, N, (), "t+1", K=16 * ks - 9, **({"act_cols": 16 * ks - 16} if aol else {})))      # K not in whole steps, not padded
            if not aol:
                fam.append(_mk(inst, "dgrad", ks, N, (), "t+1", accumulate=True))
            cases += fam
    # the W = 64 layers: two n-tiles are no whole group of four
    cases.append(_mk(Inst(GENERAL, 4, 0, 0, 0, 1), "fwd", 4, 64, (), "ragged"))
    cases.append(_mk(Inst(GENERAL, 4, 0, 1, 0, 1), "fwd", 4, 64, (), "t+1"))
    cases.append(_mk(Inst(GENERAL, 4, 0, 0, 1, 1), "dgrad", 4, 64, (), "t+1"))
    # the full-tile shapes with SNERF_GEMM_FULL=0
    cases.append(_mk(Inst(GENERAL, 4, 0, 0, 0, 1), "fwd", 16, 256, _sw(full=0), "t+1"))
    # ---- gemm_rows16_kernel<NT, PF, AOL, ACT>, counted in 32-k steps s: NT = 8 (128 columns) for s = 1..9, NT = 4 (64 columns, forward only) for s = 11..19
    # and, with a table, s = 10.  PF = 4: a table and s % 4 == 0; else 2 for even s, 1 for odd s.
    for nt, N in ((8, 384), (4, 192)):
        for pf in (1, 2, 4):
            for aol, act in ((0, 0), (1, 0), (0, 1)):
                if (pf == 4 and not (aol and not act)) or (nt == 4 and act):
                    continue
                rng = range(1, 10) if nt == 8 else range(10 if aol else 11, 20)
                ok = lambda s: (pf == 4 and s % 4 == 0) or (pf == 2 and s % 2 == 0 and not (aol and s % 4 == 0)) or (pf == 1 and s % 2 == 1)
                allowed = [2 * s for s in rng if ok(s)]
                cases += _family(Inst(ROWS16, nt, pf, aol, act, 1), allowed, N, lambda ks: ())
    # ---- gemm_areg_kernel<NT, AOL, PFA, ACT, HV>: N = 512 (NT = 16; forward by default as HV = 2 with NT = 8 per column half, PFA = 4) or N = 256 (NT = 8;
    # by default only for K > 256, SNERF_GEMM_AREG=2 below); k-steps a multiple of 4 from 8 on, PFA = 8 where they are a multiple of 8, else 4
    for aol in (0, 1):
        cases += _family(Inst(AREG, 8, 4, aol, 0, 2), [k for k in range(8, 37, 4)], 512, lambda ks: ())
    for pf in (8, 4):
        allowed = [k for k in range(8, 37, 4) if (k % 8 == 0) == (pf == 8)]
        for aol in (0, 1):
            cases += _family(Inst(AREG, 16, pf, aol, 0, 1), allowed, 512, lambda ks: _sw(areg_hv=1))
            cases += _family(Inst(AREG, 8, pf, aol, 0, 1), allowed, 256, lambda ks: _sw(areg=2) if ks <= 16 else ())
        cases += _family(Inst(AREG, 16, pf, 0, 1, 1), allowed, 512, lambda ks: ())
        cases += _family(Inst(AREG, 8, pf, 0, 1, 1), allowed, 256, lambda ks: _sw(areg=2) if ks <= 16 else ())
    return cases


CASES = _build()
COVERED = sorted(set(c.inst for c in CASES))


def cases_of(inst):
    return [c for c in CASES if c.inst == inst]
