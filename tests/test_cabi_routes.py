"""CPU-only characterisation of the host routing in csrc/api.cpp: which packed program a model holds for a width and precision (snerf_model_pack_host,
snerf_model_pack_sun_walk_host), which field kernel a launch would get (snerf_field_kernel_info) and which error a wrong call gets, code and message.

The expected values are literals, recorded from the build before the model object's programs became one table; host code that routes differently
changes one of them.  Weights: the oracle's init law, seed 0, C = 4 -
`auto` resolves to int8 digits for them (tests/test_cabi_host.py::test_auto_precision_follows_the_error_bound).  No device: nothing is finalized, the CU
count of snerf_field_kernel_info falls back to 256."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:      # imported by the child processes below
    sys.path.insert(0, REPO)
from oracle import season_nerf_oracle as orc      # noqa: E402
from test_surface_host import built      # noqa: E402,F401  (the session fixture)

WIDTHS = (64, 256, 512)
PRECISIONS = {"bf16x3": 0, "bf16": 1, "i8x3": 2, "auto": 3}
N_POINTS = (1, 64, 65, 128, 129, 256, 257, 10 ** 6)      # 1, one tile and one tile + 1 of every kernel family (64: K-split, 128: bf16 and one-wave int8, 256: two-wave int8), 10^6

_sd = {}


def _lib():
    import season_nerf_amd as sn
    return sn._lib.lib()


def _model(L, W, precision, without=()):
    m = L.snerf_model_create(W, 4)
    assert m and L.snerf_model_set_precision(m, PRECISIONS[precision]) == 0
    if W not in _sd:
        _sd[W] = {k.encode(): np.ascontiguousarray(v.numpy(), dtype=np.float32) for k, v in orc.init_weights(W, 4, 0).items() if v.is_floating_point()}
    for k, a in _sd[W].items():
        if k not in without:
            assert L.snerf_model_set_tensor(m, k, a.ctypes.data, a.size) == 0
    return m


def _err(L):
    return L.snerf_last_error().decode()


def pack_host(L, m, prog):
    """(0, stream bytes, table floats, sha256 of stream then table) or (code, message)"""
    ns, nb = C.c_size_t(), C.c_size_t()
    rc = L.snerf_model_pack_host(m, prog, None, C.byref(ns), None, C.byref(nb))
    if rc:
        return rc, _err(L)
    s, b = np.zeros(ns.value, np.uint8), np.zeros(nb.value, np.float32)
    assert L.snerf_model_pack_host(m, prog, s.ctypes.data, C.byref(ns), b.ctypes.data, C.byref(nb)) == 0 and (ns.value, nb.value) == (s.size, b.size)
    return 0, s.size, b.size, hashlib.sha256(s.tobytes() + b.tobytes()).hexdigest()


def pack_sun_walk(L, m, n_suns):
    ns = C.c_size_t()
    rc = L.snerf_model_pack_sun_walk_host(m, n_suns, None, C.byref(ns))
    if rc:
        return rc, _err(L)
    s = np.zeros(ns.value, np.uint8)
    assert L.snerf_model_pack_sun_walk_host(m, n_suns, s.ctypes.data, C.byref(ns)) == 0 and ns.value == s.size
    return 0, s.size, hashlib.sha256(s.tobytes()).hexdigest()


def kernel_info(L, m, n):
    g, b, l = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    rc = L.snerf_field_kernel_info(m, n, C.byref(g), C.byref(b), C.byref(l))
    return (rc, _err(L)) if rc else (g.value, b.value, l.value)


def measure_pack(L):
    """a fresh model per program: what a cold snerf_model_pack_host packs and answers"""
    out = {}
    for W in WIDTHS:
        for prec in PRECISIONS:
            for prog in range(6):
                m = _model(L, W, prec)
                out[W, prec, prog] = pack_host(L, m, prog)
                L.snerf_model_destroy(m)
    return out


def measure_sun_walk(L):
    out = {}
    for W, prec in [(64, "bf16x3"), (256, "bf16x3"), (512, "bf16x3"), (64, "i8x3")]:
        m = _model(L, W, prec)
        for n_suns in (1, 3, 32, 0, 33):
            out[W, prec, n_suns] = pack_sun_walk(L, m, n_suns)
        L.snerf_model_destroy(m)
    return out


def measure_info(L, combos=None):
    out = {}
    for W, prec in combos or [(W, p) for W in WIDTHS for p in PRECISIONS]:
        m = _model(L, W, prec)
        for n in N_POINTS:
            out[W, prec, n] = kernel_info(L, m, n)
        L.snerf_model_destroy(m)
    return out


def measure_refusals(L):
    """Every entry point that takes a model: NULL model, un-finalized model, each class of bad argument it names - and, where model and argument are both
    bad, which of the two it reports.  Nothing gets as far as a pointer: any aligned address will do."""
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 63) & ~63
    sun3 = (C.c_double * 3)(0.3, -0.2, 0.8)
    s3 = C.addressof(sun3)
    import season_nerf_amd as sn
    est = C.byref(sn._lib.I8Estimate())
    U = _model(L, 64, "bf16x3")               # complete, not finalized
    # one tensor missing (with more than one gone, which of them a program's packer names depends on its worker threads)
    E = _model(L, 64, "bf16x3", without=(b"G_NeRF_net.fc1.linear.weight",))
    out = {}

    def case(name, rc):
        out[name] = (rc, _err(L) if rc < 0 else "")

    def each(name, fn, good, bad):
        """good: arguments after the model; bad: {label: (index, value)}.  Both models with good arguments, every bad argument with the un-finalized and the
        NULL model (the doubly wrong calls)."""
        case(name + "/null", fn(None, *good))
        case(name + "/unfinalized", fn(U, *good))
        for label, (i, v) in bad.items():
            a = list(good)
            a[i] = v
            case(f"{name}/{label}+unfinalized", fn(U, *a))
            case(f"{name}/{label}+null", fn(None, *a))

    case("set_precision/null", L.snerf_model_set_precision(None, 0))
    case("set_precision/unknown", L.snerf_model_set_precision(E, 7))
    case("set_precision/null+unknown", L.snerf_model_set_precision(None, 7))
    out["precision/null"] = (L.snerf_model_precision(None), "")
    out["width/null"] = (L.snerf_model_width(None), "")
    out["classes/null"] = (L.snerf_model_classes(None), "")
    case("i8_estimate/null", L.snerf_model_i8_estimate(None, est))
    case("i8_estimate/null_out", L.snerf_model_i8_estimate(U, None))
    case("i8_estimate/one_missing", L.snerf_model_i8_estimate(E, est))
    case("set_tensor/null", L.snerf_model_set_tensor(None, b"x", p, 4))
    case("set_tensor/null_key", L.snerf_model_set_tensor(E, None, p, 4))
    case("set_tensor/null_data", L.snerf_model_set_tensor(E, b"x", None, 4))
    case("resolve/null", L.snerf_model_resolve_precision(None))
    case("resolve/one_missing", L.snerf_model_resolve_precision(E))
    case("finalize/null", L.snerf_model_finalize(None))
    case("finalize/one_missing", L.snerf_model_finalize(E))
    n = C.c_size_t()
    for prog in (-1, 6):
        case(f"pack_host/program{prog}", L.snerf_model_pack_host(U, prog, None, C.byref(n), None, None))
        case(f"pack_host/program{prog}+null", L.snerf_model_pack_host(None, prog, None, C.byref(n), None, None))
    case("pack_host/null", L.snerf_model_pack_host(None, 0, None, C.byref(n), None, None))
    case("pack_host/one_missing", L.snerf_model_pack_host(E, 0, None, C.byref(n), None, None))
    case("pack_host/one_missing_program2", L.snerf_model_pack_host(E, 2, None, C.byref(n), None, None))      # the E_STATE refusal comes before the packer's
    case("pack_sun_walk/null", L.snerf_model_pack_sun_walk_host(None, 3, None, C.byref(n)))
    case("pack_sun_walk/null+n_suns0", L.snerf_model_pack_sun_walk_host(None, 0, None, C.byref(n)))
    case("pack_sun_walk/one_missing", L.snerf_model_pack_sun_walk_host(E, 3, None, C.byref(n)))
    case("pack_sun_walk/one_missing+n_suns33", L.snerf_model_pack_sun_walk_host(E, 33, None, C.byref(n)))
    for W in (64, 512):      # a field and a per-ray tensor missing: the field program is packed first, whichever program is asked for
        D = _model(L, W, "bf16x3", without=(b"time_layer_1.linear.weight", b"G_NeRF_net.fc2.linear.weight"))
        case(f"resolve/two_missing_W{W}", L.snerf_model_resolve_precision(D))
        case(f"pack_host/two_missing_W{W}_program1", L.snerf_model_pack_host(D, 1, None, C.byref(n), None, None))
        L.snerf_model_destroy(D)
    case("kernel_info/null", L.snerf_field_kernel_info(None, 1, None, None, None))
    case("kernel_info/one_missing", L.snerf_field_kernel_info(E, 1, None, None, None))

    each("group_forward", L.snerf_group_forward, [4, p, p, p, p, p, None], {"n<0": (0, -1), "time": (1, None), "sun": (2, None), "n=0": (0, 0)})
    each("forward_points", L.snerf_field_forward_points, [0, 4, p, 1, p, p, None, None],
         {"variant": (0, 4), "n<0": (1, -1), "points": (2, None), "group_size": (3, 0), "n=0": (1, 0)})
    each("forward_rays", L.snerf_field_forward_rays, [0, 4, 8, p, p, p, 1, p, p, None, None],
         {"variant": (0, 4), "n<0": (1, -1), "samples": (2, 0), "top": (3, None), "bot": (4, None), "tvals": (5, None), "rays_per_group": (6, 0), "n=0": (1, 0)})
    each("ray_visibility", L.snerf_field_ray_visibility, [4, 8, p, p, p, 0, p, None],
         {"n<0": (0, -1), "samples": (1, 0), "top": (2, None), "bot": (3, None), "tvals": (4, None), "vis": (6, None), "n=0": (0, 0)})
    each("sun_walk", L.snerf_field_sun_walk_rays, [4, 8, p, p, p, 3, p, p, None, None],
         {"n<0": (0, -1), "samples": (1, 0), "top": (2, None), "bot": (3, None), "tvals": (4, None), "n_suns0": (5, 0), "n_suns33": (5, 33), "suns": (6, None),
          "n=0": (0, 0)})
    each("ray_surface", L.snerf_field_ray_surface, [4, 8, p, p, p, 0, p, None],
         {"n<0": (0, -1), "samples": (1, 0), "top": (2, None), "bot": (3, None), "tvals": (4, None), "out": (6, None), "out_align": (6, p + 8), "n=0": (0, 0)})
    each("shadow_walk", L.snerf_field_shadow_walk, [4, 8, p, p, p, p, 0, p, None],
         {"n<0": (0, -1), "samples": (1, 0), "top": (2, None), "bot": (3, None), "sun": (4, None), "tvals": (5, None), "out": (7, None), "out_align": (7, p + 16),
          "n=0": (0, 0)})
    bad_sun = (C.c_double * 3)(0.3, -0.2, 0.0)
    each("solar_audit", L.snerf_field_solar_audit, [4, 8, p, p, p, s3, p, p, 2, p, None, None],
         {"n<0": (0, -1), "samples": (1, 0), "top": (2, None), "bot": (3, None), "tvals": (4, None), "sun_null": (5, None), "sun_z": (5, C.addressof(bad_sun)),
          "est_vis": (6, None), "ps": (7, None), "flags": (8, 1), "out": (9, None), "out_align": (9, p + 16), "n=0": (0, 0)})
    each("frame_walk", L.snerf_field_frame_walk, [4, 8, p, p, p, 0.5, p, p, 2, p, 0, p, None],
         {"n<0": (0, -1), "samples": (1, 1), "top": (2, None), "bot": (3, None), "tvals": (4, None), "delta0": (5, 0.0), "delta_nan": (5, float("nan")),
          "sun": (6, None), "sky": (7, None), "n_times0": (8, 0), "n_times5": (8, 5), "class_vecs": (9, None), "out": (11, None), "out_align": (11, p + 32),
          "n=0": (0, 0)})
    each("render_rays", L.snerf_render_rays, [4, 8, p, p, p, p, p, 0, p, None, None, p, 1 << 20, None],
         {"n<0": (0, -1), "samples": (1, 0), "top": (2, None), "sun": (5, None), "time": (6, None), "workspace": (10, None), "workspace_small": (11, 16),
          "n=0": (0, 0)})
    L.snerf_model_destroy(U)
    L.snerf_model_destroy(E)
    return out


_ENV_CHILD = r"""
import sys
sys.path.insert(0, %r)
import test_cabi_routes as t
L = t._lib()
print(repr(t.measure_info(L, [(256, "i8x3"), (64, "i8x3")])))
"""


def measure_info_under(switch):
    """snerf_field_kernel_info of the int8 models with an A/B switch set: a child process, as the switches are read once"""
    r = subprocess.run([sys.executable, "-c", _ENV_CHILD % os.path.join(REPO, "tests")], env=dict(os.environ, **{switch: "1"}), capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return eval(r.stdout.strip().splitlines()[-1])


# ---------------------------------------------------------------------------------------------------------------------------------------------------------
# recorded values
# a packed program does not depend on the precision it was asked for under: (width, program) -> (stream bytes, table floats, sha256 of stream then table)
PROGRAMS = {
    (64, 0): (311296, 928, "2a94a0ca509a6b61a41db32f8e0ae7932c83dd51aacec2815102553dd5eb72e5"),
    (64, 1): (81920, 224, "1b150c46440dfdbed9ee4e2a5880a7e3e2521b4ca9578065545ed353806188db"),
    (64, 2): (294912, 2336, "99b066262feb19d14e12a12f9515b2e3a7f033952d380dd0eb379f5c51d4e9bc"),
    (256, 0): (3031040, 3424, "049a656807ebe2858b55b031d826ccee5df1bd5ce19e8c9c8944e15cc96e56c8"),
    (256, 1): (360448, 640, "abf3b7f91d8791a19d1f05aee7f3d111b72b0547489ce553ae6a20191fcba2c6"),
    (256, 2): (1540096, 8768, "95af6a30d3d6eb369e2702162752015009a0abe39957906ef378bfeda5bea7ac"),
    (256, 5): (1540096, 8672, "989cb26620afcdaab216618a8267acec5084141996cc5dbd2d0faebc1c864a41"),
    (512, 0): (11698176, 6752, "3b41d5d47e51001f914a38163ef150dc7dc5a939753ab3e7cfa98c322bf9f0d8"),
    (512, 1): (1212416, 1216, "c29de70e9b79b4f29ef4008cb6b95b1c94dd01c53a3febc0cca2192fe5151e2d"),
    (512, 2): (5849088, 17344, "b307f3bb24de17423cc32bd8a0a303eb8d724753ec8b7d997e38e744c025486f"),
    (512, 3): (11698176, 6752, "67be97bd820be4de1a098a4e5faea442015ac3e41ee6531223cf7ead6a7a250b"),
    (512, 4): (1212416, 1216, "191e72a09e466db825be4ef96baf57520f4d80b00b73cdcd9881de0a491e736a"),
}
# return code of a cold snerf_model_pack_host per program 0..5 (an unresolved `auto` is not yet SNERF_PREC_I8X3: programs 2 and 5 are refused)
PACK_CODES = {
    (64, "bf16x3"): (0, 0, -4, -4, -4, -4), (64, "bf16"): (0, 0, -4, -4, -4, -4), (64, "i8x3"): (0, 0, 0, -4, -4, -4), (64, "auto"): (0, 0, -4, -4, -4, -4),
    (256, "bf16x3"): (0, 0, -4, -4, -4, -4), (256, "bf16"): (0, 0, -4, -4, -4, -4), (256, "i8x3"): (0, 0, 0, -4, -4, 0), (256, "auto"): (0, 0, -4, -4, -4, -4),
    (512, "bf16x3"): (0, 0, -4, 0, 0, -4), (512, "bf16"): (-1, -1, -4, -1, -1, -4), (512, "i8x3"): (0, 0, 0, 0, 0, -4), (512, "auto"): (0, 0, -4, 0, 0, -4),
}
NO_PROGRAM = {2: "program 2 (int8-digit field network) exists only under SNERF_PREC_I8X3",
              3: "program 3 (K-split bf16 field network) exists only at width 512",
              4: "program 4 (K-split per-ray networks) exists only at width 512",
              5: "program 5 (int8 digits for the 16x16x64 matrix instruction) exists only under SNERF_PREC_I8X3 at width 256"}
NO_KERNEL_512 = "layer_width 512 has fused kernels only under SNERF_PREC_I8X3 and SNERF_PREC_BF16X3"
EXPECTED_PACK = {(W, prec, prog): (0,) + PROGRAMS[W, prog] if rc == 0 else (rc, NO_PROGRAM[prog] if rc == -4 else NO_KERNEL_512)
                 for (W, prec), codes in PACK_CODES.items() for prog, rc in enumerate(codes)}

N_SUNS_RANGE = "snerf_model_pack_sun_walk_host: n_suns must be in [1,32]"
WALK_STREAMS = {      # (width, n_suns) -> (bytes, sha256): the same under bf16x3 and i8x3
    (64, 1): (311296, "a7bca77e2c3db7bee152b29bef56d5ba7959a75c21834645ebf4046b6882f96e"),
    (64, 3): (442368, "83bd625f9a426deae24bc5ff4dd087e9e46a30d51635274b5cdb81a0304f0251"),
    (64, 32): (2342912, "604007552fb969f557b01aa845beeb778d4391f6d5d2a22ad1104e4976435578"),
    (256, 1): (3031040, "caa1b4419e32b354c822b54d022b1a531f2b10f5c5a4d4f419611745b7c98157"),
    (256, 3): (3489792, "718ebb11d9ff6fdfe584eaaad665d5edcf2b84a4ad0496393e32374eb90b1521"),
    (256, 32): (10141696, "170a007f1c2a5a3612e7a9cc6cf1c109c629c50b47dc42fb4ee89c3f09f29888"),
    (512, 1): (11698176, "9a53358b1590408f18839e1d5b195b2b6726e6667f9deb3cd2c7cfc0e3ffadc3"),
    (512, 3): (13402112, "fc26098fb0d8062099e850e3e2e2d1236b89c1340e406179604e7d8f77f8151d"),
    (512, 32): (38109184, "86fca6da4463d8351ecfcb6742e7b9b3aa9de497d5ada0715ddc1dd5f1def7d1"),
}
EXPECTED_SUN_WALK = {(W, prec, n): (0,) + WALK_STREAMS[W, n] if 1 <= n <= 32 else (-1, N_SUNS_RANGE)
                     for W, prec in [(64, "bf16x3"), (256, "bf16x3"), (512, "bf16x3"), (64, "i8x3")] for n in (1, 3, 32, 0, 33)}

# snerf_field_kernel_info: (width, precision) -> (grid at each of N_POINTS, block, lds_bytes)
GRID_128 = (1, 1, 1, 1, 2, 2, 3, 256)      # tiles of 128 points: the bf16 kernels and the one-wave int8 kernel
GRID_256 = (1, 1, 1, 1, 1, 1, 2, 256)      # tiles of 256: the two-wave int8 kernel
GRID_64 = (1, 1, 2, 2, 3, 4, 5, 256)       # tiles of 64: the K-split kernel
INFO = {
    (64, "bf16x3"): (GRID_128, 256, 118464), (64, "bf16"): (GRID_128, 256, 118464), (64, "i8x3"): (GRID_256, 512, 124096), (64, "auto"): (GRID_256, 512, 124096),
    (256, "bf16x3"): (GRID_128, 256, 128448), (256, "bf16"): (GRID_128, 256, 128448), (256, "i8x3"): (GRID_256, 512, 149440), (256, "auto"): (GRID_256, 512, 149440),
    (512, "bf16x3"): (GRID_64, 256, 158272), (512, "bf16"): None, (512, "i8x3"): (GRID_128, 256, 151360), (512, "auto"): (GRID_128, 256, 151360),
}
INFO_ONE_WAVE = {(256, "i8x3"): (GRID_128, 256, 149824), (64, "i8x3"): (GRID_128, 256, 124096)}      # SNERF_I8_ONE_WAVE=1: kernels_i8.hip, the 32x32x32 tables
INFO_MFMA32 = {(256, "i8x3"): (GRID_256, 512, 149824), (64, "i8x3"): (GRID_256, 512, 124096)}        # SNERF_I8X2_MFMA32=1: two waves, the 32x32x32 tables


def _info(table):
    return {(W, prec, n): (row[0][i], row[1], row[2]) if row else (-1, NO_KERNEL_512) for (W, prec), row in table.items() for i, n in enumerate(N_POINTS)}


EXPECTED_INFO, EXPECTED_INFO_ONE_WAVE, EXPECTED_INFO_MFMA32 = _info(INFO), _info(INFO_ONE_WAVE), _info(INFO_MFMA32)

NULL_MODEL, NOT_FINALIZED = (-1, "NULL model"), (-4, "model not finalized (call snerf_model_finalize)")
MISSING = (-2, "missing tensor: G_NeRF_net.fc1.linear.weight")
REFUSALS = {
    "set_precision/null": NULL_MODEL, "set_precision/unknown": (-1, "unknown precision mode 7"), "set_precision/null+unknown": NULL_MODEL,
    "precision/null": (-1, ""), "width/null": (0, ""), "classes/null": (0, ""),
    "i8_estimate/null": (-1, "snerf_model_i8_estimate: NULL argument"), "i8_estimate/null_out": (-1, "snerf_model_i8_estimate: NULL argument"),
    "i8_estimate/one_missing": MISSING,
    "set_tensor/null": (-1, "snerf_model_set_tensor: NULL argument"), "set_tensor/null_key": (-1, "snerf_model_set_tensor: NULL argument"),
    "set_tensor/null_data": (-1, "snerf_model_set_tensor: NULL argument"),
    "resolve/null": NULL_MODEL, "resolve/one_missing": MISSING, "finalize/null": NULL_MODEL, "finalize/one_missing": MISSING,
    "pack_host/program-1": (-1, "snerf_model_pack_host: bad argument"), "pack_host/program-1+null": (-1, "snerf_model_pack_host: bad argument"),
    "pack_host/program6": (-1, "snerf_model_pack_host: bad argument"), "pack_host/program6+null": (-1, "snerf_model_pack_host: bad argument"),
    "pack_host/null": (-1, "snerf_model_pack_host: bad argument"), "pack_host/one_missing": MISSING, "pack_host/one_missing_program2": (-4, NO_PROGRAM[2]),
    "pack_sun_walk/null": NULL_MODEL, "pack_sun_walk/null+n_suns0": NULL_MODEL, "pack_sun_walk/one_missing": MISSING,
    "pack_sun_walk/one_missing+n_suns33": (-1, N_SUNS_RANGE),
    "kernel_info/null": NULL_MODEL, "kernel_info/one_missing": MISSING,
    "resolve/two_missing_W64": (-2, "missing tensor: G_NeRF_net.fc2.linear.weight"), "pack_host/two_missing_W64_program1": (-2, "missing tensor: G_NeRF_net.fc2.linear.weight"),
    "resolve/two_missing_W512": (-2, "missing tensor: G_NeRF_net.fc2.linear.weight"), "pack_host/two_missing_W512_program1": (-2, "missing tensor: G_NeRF_net.fc2.linear.weight"),
}
# The launching entry points.  Those that look at the model first answer every wrong argument with the model's state; the others name the argument first:
# name -> (labels of measure_refusals, answer to a NULL model with good arguments, answer to a bad argument or None = the model's state, exceptions)
SOLAR_AUDIT = "snerf_field_solar_audit: bad argument (n_rays >= 0, n_samples >= 1, no NULL pointer but d_exact, d_out 32-byte aligned)"
FRAME_WALK = "snerf_field_frame_walk: bad argument (n_samples >= 2, n_times in [1,4], delta finite and positive, d_out 64-byte aligned)"
LAUNCHERS = {
    "group_forward": ("n<0 time sun", NULL_MODEL, None, {}),
    "forward_points": ("variant n<0 points group_size", NULL_MODEL, None, {}),
    "forward_rays": ("variant n<0 samples top bot tvals rays_per_group", NULL_MODEL, None, {}),
    "ray_visibility": ("n<0 samples top bot tvals vis", NULL_MODEL, None, {}),
    "sun_walk": ("n<0 samples top bot tvals n_suns0 n_suns33 suns", NULL_MODEL, None, {}),
    "render_rays": ("n<0 samples top sun time workspace workspace_small", NULL_MODEL, None, {}),
    "ray_surface": ("n<0 samples top bot tvals out out_align", NULL_MODEL, (-1, "snerf_field_ray_surface: bad argument (d_out must be 16-byte aligned)"), {}),
    "shadow_walk": ("n<0 samples top bot sun tvals out out_align", NULL_MODEL, (-1, "snerf_field_shadow_walk: bad argument (d_out must be 32-byte aligned)"), {}),
    "solar_audit": ("n<0 samples top bot tvals sun_null sun_z est_vis ps flags out out_align", (-1, "snerf_field_solar_audit: NULL model"), (-1, SOLAR_AUDIT),
                    {"sun_z": (-1, "snerf_field_solar_audit: the sun direction must be finite with sun_z > 0"),
                     "flags": (-1, "snerf_field_solar_audit: flags has bits other than 2 (outside the cube: delta 0) and 4 (no early-out)")}),
    "frame_walk": ("n<0 samples top bot tvals delta0 delta_nan sun sky n_times0 n_times5 class_vecs out out_align", NULL_MODEL, (-1, FRAME_WALK), {}),
}


def _refusals():
    out = dict(REFUSALS)
    for name, (labels, null, bad, other) in LAUNCHERS.items():
        out[name + "/null"], out[name + "/unfinalized"] = null, NOT_FINALIZED
        for label in labels.split() + ["n=0"]:      # no rays: not wrong, and answered after the model's state everywhere
            first = None if label == "n=0" else other.get(label, bad)
            out[f"{name}/{label}+unfinalized"], out[f"{name}/{label}+null"] = first or NOT_FINALIZED, first or null
    return out


EXPECTED_REFUSALS = _refusals()


def _same(got, want):
    assert sorted(got) == sorted(want)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, bad


def test_pack_host_of_every_program(built):      # noqa: F811
    L = _lib()
    _same(measure_pack(L), EXPECTED_PACK)
    assert len(EXPECTED_PACK) == 72
    # refusals: programs that do not exist for the combination are SNERF_E_STATE, the fast mode at 512 SNERF_E_INVALID for every program it has
    assert all(EXPECTED_PACK[512, "bf16", p][0] == (-4 if p in (2, 5) else -1) for p in range(6))
    assert all(EXPECTED_PACK[W, "bf16x3", 2][0] == -4 and EXPECTED_PACK[W, "bf16x3", 5][0] == -4 for W in WIDTHS)
    assert [W for W in WIDTHS if EXPECTED_PACK[W, "i8x3", 5][0] == 0] == [256]


def test_pack_host_on_one_model_in_any_order(built):      # noqa: F811
    """What one model answers does not depend on which program was asked for first (each packs what it lacks); `auto` answers as the mode it resolved to."""
    L = _lib()
    for W in WIDTHS:
        for prec in ("bf16x3", "i8x3", "auto"):
            for order in (range(6), range(5, -1, -1)):
                m = _model(L, W, prec)
                r = L.snerf_model_resolve_precision(m)
                assert r == PRECISIONS["i8x3" if prec == "auto" else prec]
                for prog in list(order) * 2:
                    assert pack_host(L, m, prog) == EXPECTED_PACK[W, "i8x3" if prec == "auto" else prec, prog], (W, prec, prog)
                L.snerf_model_destroy(m)


def test_pack_sun_walk_host(built):      # noqa: F811
    _same(measure_sun_walk(_lib()), EXPECTED_SUN_WALK)


def test_field_kernel_info(built):      # noqa: F811
    _same(measure_info(_lib()), EXPECTED_INFO)
    assert len(EXPECTED_INFO) == 12 * len(N_POINTS)


@pytest.mark.parametrize("switch", ["SNERF_I8_ONE_WAVE", "SNERF_I8X2_MFMA32"])
def test_field_kernel_info_under_the_ab_switches(built, switch):      # noqa: F811
    want = {"SNERF_I8_ONE_WAVE": EXPECTED_INFO_ONE_WAVE, "SNERF_I8X2_MFMA32": EXPECTED_INFO_MFMA32}[switch]
    _same(measure_info_under(switch), want)
    assert any(want[k] != EXPECTED_INFO[k] for k in want)      # the switch routes somewhere else


def test_refusals(built):      # noqa: F811
    _same(measure_refusals(_lib()), EXPECTED_REFUSALS)

