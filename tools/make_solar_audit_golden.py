#!/usr/bin/env python
"""Generate tests/golden/solar_audit.npz by running the REFERENCE itself: `component_render_by_dir(..., include_exact_solar=True)`
(T_NeRF_Eval_Utils/mg_Img_Eval.py:17-72,96-115) and `eval_solar_data` / `_get_stats` (T_NeRF_Eval_Utils/mg_Advanced_Solar.py:11-37,79-93) on a 10 x 12
lattice, at 40 and at 96 samples per ray, for two views, three suns and four weight sets: 48 renders.  Modelled on tools/make_shadow_golden.py: the reference
imports, stubs and weight set-up of tools/make_golden.py and the `sharp_state` recipe of make_height_golden are reused; nothing of the reference is copied.
Needs a CPU and the reference checkout only (about ten minutes).

    python tools/make_solar_audit_golden.py [--full FILE]     # run the reference (or read FILE, the record of an earlier run), check, write the fixture
    python tools/make_solar_audit_golden.py --check            # the band conditions on the fixture as it stands
--full FILE keeps every per-sample array of all 48 renders (2.9 MB, outside the repository): the selection below can then be redone without the reference,
e.g. after the bands of tests/test_audit_host.py were measured anew.

What is stored (the views, suns, sample counts and `ARRAYS`, the renders kept per sample, are those of tests/test_audit_host.py):
    tags, S_list, lattice (H, W), views [2,2] and sun_el_az [3,2] (el, az in degrees), W2C, W2L_H, sun_vecs [3,3] (world_angle_2_local_vec, float64)
    for every render, stacked in the order of `renders()` of tests/test_audit_host.py (tag, S, view, sun):
      confusion    [48,2,4] int64     eval_solar_data: All_Solar_Vis and Surface_Solar_Vis, each TP, TN, FP, FN
      stats        [48,2,9] float64   _get_stats of the two rows
    for the renders of ARRAYS, per sample, as float32 (the reference computes them in fp32; its float64 arrays hold these values):
      {tag}_S{S}_v{v}_s{s}_Exact_Solar, _Est_Solar_Vis [R,S];  {tag}_S{S}_v{v}_Rho, _Deltas [R,S] (they do not depend on the sun: recorded once per view)
    for the other renders, what the comparisons on the device need of the per-sample arrays (all 48 per sample are 2.9 MB; the fixture may not be larger than
    shadow_points.npz):
      surf         [48,2,R] float64   sum_s Exact PS and sum_s Est PS per ray, PS as eval_solar_data forms it (float64); NaN for the renders of ARRAYS
      near         [2,N] float32      |Exact - .5| and |Est - .5| of the samples where either is below NEAR, render i at near_start[i] .. near_start[i+1]
The band conditions of tests/test_audit_host.py (band_conditions) are asserted before the file is written, and NEAR must cover the band: a fixture that
cannot carry the test is never written.  Weight sets: init_W64_s2 (the init law, seed 2) and sharp_W64 / sharp_W256 / sharp_W512, as in
tools/make_height_golden.py.
"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import test_audit_host as T      # noqa: E402  (the views, suns and sample counts, the selection and the band conditions)

LATTICE = (10, 12)
OUT = os.path.join(REPO, "tests", "golden")
PATH = os.path.join(OUT, "solar_audit.npz")
PER_SAMPLE = ("Rho", "Deltas", "Exact_Solar", "Est_Solar_Vis")


def run_reference():
    """Every render of the fixture -> the full record: header, and per render the four per-sample arrays, the confusion dicts and the statistics."""
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import make_golden as mg      # noqa: E402  (stubs the reference's optional imports and puts it on sys.path)
    from make_height_golden import sharp_state
    from T_NeRF_Eval_Utils.mg_Advanced_Solar import _get_stats, eval_solar_data
    out = {"tags": np.array(T.TAGS), "S_list": np.array(T.S_LIST), "lattice": np.array(LATTICE), "views": np.array(T.VIEWS), "sun_el_az": np.array(T.SUN_EL_AZ),
           "W2C": mg.WC, "W2L_H": mg.H4, "sun_vecs": np.array([mg.world_angle_2_local_vec(a[0], a[1], mg.WC, mg.H4) for a in T.SUN_EL_AZ], dtype=np.float64)}
    nets = {"init_W64_s2": mg.make_net(64, 4, 2)[0]}
    for W in (64, 256, 512):
        net = mg.T_NeRF(W, 4)
        r = net.load_state_dict(sharp_state(W), strict=True)
        assert not r.missing_keys and not r.unexpected_keys
        nets[f"sharp_W{W}"] = net
    f32 = lambda a: np.ascontiguousarray(a[..., 0].astype(np.float32))
    for tag, S, vi, si, k in T.renders():
        net = nets[tag].eval()
        with np.errstate(divide="ignore", invalid="ignore"):
            d = mg.component_render_by_dir(net, T.VIEWS[vi], T.SUN_EL_AZ[si], 0.0, (LATTICE[0], LATTICE[1], S), mg.WC, mg.H4, torch.device("cpu"), include_exact_solar=True)
            conf = eval_solar_data(d)
            stats = [_get_stats(*(conf[fam][c] for c in T.CONF_KEYS)) for fam in T.FAMILIES]
        kv = T.key_of(tag, S, vi)
        for name in PER_SAMPLE:
            assert np.array_equal(f32(d[name]).astype(np.float64), d[name][..., 0]), name      # fp32 values: nothing lost
        for name in ("Rho", "Deltas"):
            if si == 0:
                out[f"{kv}_{name}"] = f32(d[name])
            assert np.array_equal(out[f"{kv}_{name}"], f32(d[name])), name
        out[k + "_Exact_Solar"], out[k + "_Est_Solar_Vis"] = f32(d["Exact_Solar"]), f32(d["Est_Solar_Vis"])
        out[k + "_confusion"] = np.array([[int(conf[fam][c]) for c in T.CONF_KEYS] for fam in T.FAMILIES], dtype=np.int64)
        out[k + "_stats"] = np.array(stats, dtype=np.float64)
        print(f"{k}: All {conf['All_Solar_Vis']}  Surface {conf['Surface_Solar_Vis']}", flush=True)
    return out


def select(full):
    """The fixture from the full record: per-sample arrays for the renders of T.ARRAYS, `surf` and `near` for the others."""
    full = T.Fixture(full)
    drop = tuple("_" + n for n in PER_SAMPLE) + ("_confusion", "_stats")
    out = {k: v for k, v in full.items() if not k.endswith(drop)}
    R = LATTICE[0] * LATTICE[1]
    conf, stats, surf, near, start = [], [], [], [], [0]
    for tag, S, vi, si, k in T.renders():
        conf.append(full[k + "_confusion"])
        stats.append(full[k + "_stats"])
        if (tag, S, vi, si) in T.ARRAYS:
            for name in ("Rho", "Deltas"):
                out[f"{T.key_of(tag, S, vi)}_{name}"] = full[f"{T.key_of(tag, S, vi)}_{name}"]
            out[k + "_Exact_Solar"], out[k + "_Est_Solar_Vis"] = full[k + "_Exact_Solar"], full[k + "_Est_Solar_Vis"]
            surf.append(np.full([2, R], np.nan))
        else:
            ex, es = full[k + "_Exact_Solar"].astype(np.float64), full[k + "_Est_Solar_Vis"].astype(np.float64)
            ps = T.ps_of(full[k + "_Rho"].astype(np.float64), full[k + "_Deltas"].astype(np.float64))
            surf.append(np.stack([(ex * ps).sum(1), (es * ps).sum(1)]))
            a, b = np.abs(ex - .5), np.abs(es - .5)
            m = (a < T.NEAR) | (b < T.NEAR)
            near.append(np.stack([a[m], b[m]]).astype(np.float32))
            assert T.confusion_of_arrays(ex, es, ps) == {fam: dict(zip(T.CONF_KEYS, (int(x) for x in full[k + "_confusion"][i]))) for i, fam in enumerate(T.FAMILIES)}
        start.append(start[-1] + (near[-1].shape[1] if (tag, S, vi, si) not in T.ARRAYS else 0))
    out["confusion"], out["stats"], out["surf"] = np.stack(conf), np.stack(stats), np.stack(surf)
    out["near"], out["near_start"] = np.concatenate(near, 1), np.array(start, dtype=np.int64)
    return out


def main():
    if "--check" in sys.argv:
        T.band_conditions(T.fixture(OUT), T.BAND, T.BAND_SURF)
        return
    keep = sys.argv[sys.argv.index("--full") + 1] if "--full" in sys.argv else None
    if keep and os.path.exists(keep):
        full = dict(np.load(keep, allow_pickle=False))
    else:
        full = run_reference()
        if keep:
            np.savez_compressed(keep, **full)
    assert T.NEAR >= 2 * T.BAND, "NEAR must cover the band with room to spare"
    out = select(full)
    T.band_conditions(T.as_fixture(out), T.BAND, T.BAND_SURF)
    tmp = PATH + ".tmp.npz"
    np.savez_compressed(tmp, **out)
    size, limit = os.path.getsize(tmp), os.path.getsize(os.path.join(OUT, "shadow_points.npz"))
    if size > limit:
        os.remove(tmp)
        sys.exit(f"the fixture would be {size} bytes, larger than shadow_points.npz ({limit}): not written")
    os.replace(tmp, PATH)
    print(PATH, size, "bytes")


if __name__ == "__main__":
    main()
