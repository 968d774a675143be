"""CPU-only checks of the sun walk (include/season_nerf_hip.h snerf_model_pack_sun_walk_host / snerf_field_sun_walk_rays): the walk stream against an
independent statement of the chunk layout, the register contract of the two walk kernels from the shipped library's metadata, the op schemas."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from oracle import season_nerf_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 16384


def _build():
    spec = importlib.util.spec_from_file_location("snerf_build", os.path.join(REPO, "season_nerf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    b.build_ops()
    return b


@pytest.fixture(scope="module")
def lib():
    _build()
    import season_nerf_amd as sn
    return sn._lib.lib()


def _layers(W):
    """(name, output blocks of 32 rows, k-steps of the hidden input, k-steps of an encoding, raw head) of the field program, in stream order (csrc/program.h
    field_layer, restated): k-steps of 16 slots; PE(pos) 4 k-steps, PE(sun) 2."""
    W2 = W // 2
    hid = lambda n: ("h", W // 32, W // 16, 0, False)
    return [("fc1", W // 32, 0, 4, False), hid(2), hid(3), hid(4), ("fc5", W // 32, W // 16, 4, False), hid(6), hid(7), hid(8),
            ("fc9", W2 // 32, W // 16, 0, False), ("head", 1, W2 // 16, 0, True),
            ("s1", W2 // 32, W2 // 16, 2, False), ("s2", W2 // 32, W2 // 16, 0, False), ("s3", W2 // 32, W2 // 16, 0, False), ("s4", 1, W2 // 16, 0, True),
            ("a1", W // 32, W2 // 16, 0, False), ("a2", W // 32, W // 16, 0, False), ("a3", W // 32, W // 16, 0, False), ("ac", 1, W // 16, 0, True)]


def _layer_chunks(W, ks_order):
    """16 KiB chunks per layer.  Canonical order: nb * (k-steps) pairs of 2 KiB, 8 to a chunk.  K-split order (width 512): per wave parity a raw head has
    half its k-steps, a hidden layer nb / 2 steps of (hidden k-steps + encoding k-steps), an encoding-only layer nb / 2 steps of its k-steps; 4 pairs per
    parity to a chunk.  Every layer starts on a chunk boundary."""
    out = []
    for _, nb, kh, kx, raw in _layers(W):
        if not ks_order:
            out.append(-(-(nb * (kh + kx)) // 8))
        else:
            pairs = kh // 2 if raw else (nb // 2) * (kh + kx)
            out.append(-(-pairs // 4))
    return out


def _rearranged(stream, W, M, ks_order):
    ch = _layer_chunks(W, ks_order)
    assert len(stream) == sum(ch) * CHUNK
    a, b = sum(ch[:10]) * CHUNK, sum(ch[:14]) * CHUNK        # the solar layers are layers 10 .. 13
    return stream[:a] + stream[a:b] * M + stream[b:]


@pytest.mark.parametrize("W", [64, 256, 512])
def test_walk_stream_is_the_chunk_rearrangement_of_the_packed_stream(lib, W):
    m = lib.snerf_model_create(W, 4)
    assert m
    try:
        for k, v in orc.init_weights(W, 4, 3).items():
            if v.is_floating_point():
                arr = np.ascontiguousarray(v.numpy())
                assert lib.snerf_model_set_tensor(m, k.encode(), arr.ctypes.data, arr.size) == 0
        prog = 3 if W == 512 else 0
        n = C.c_size_t()
        assert lib.snerf_model_pack_host(m, prog, None, C.byref(n), None, None) == 0
        base = np.zeros(n.value, dtype=np.uint8)
        assert lib.snerf_model_pack_host(m, prog, base.ctypes.data, C.byref(n), None, None) == 0
        base = base.tobytes()
        for M in (1, 3, 32):
            q = C.c_size_t()
            assert lib.snerf_model_pack_sun_walk_host(m, M, None, C.byref(q)) == 0           # NULL size query
            want = _rearranged(base, W, M, W == 512)
            assert q.value == len(want) and q.value < 2 ** 32, (W, M, q.value)
            got = np.zeros(q.value, dtype=np.uint8)
            assert lib.snerf_model_pack_sun_walk_host(m, M, got.ctypes.data, C.byref(q)) == 0
            assert got.tobytes() == want, (W, M)
        assert _rearranged(base, W, 1, W == 512) == base                                      # one sun: the stream as packed
        for M in (0, 33, -1):
            assert lib.snerf_model_pack_sun_walk_host(m, M, None, C.byref(q)) == -1, M        # SNERF_E_INVALID
            assert b"n_suns" in lib.snerf_last_error()
    finally:
        lib.snerf_model_destroy(m)


@pytest.fixture(scope="module")
def walk_kernels():
    """Code-object metadata of the walk kernels in the shipped library, by width (read as tests/test_group_split_code_object.py reads it)."""
    b = _build()
    spec = importlib.util.spec_from_file_location("snerf_isa_guards", os.path.join(REPO, "tests", "test_isa_guards.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    walk, walk_ks = {}, {}
    for elf in g._device_code_objects(b.LIB):
        for k in g._kernel_metadata(elf):
            m = re.match(r"_ZN5snerf\d+sun_walk_kernelILi(\d+)EEEv", k[".name"])
            if m:
                walk[int(m.group(1))] = k
            m = re.match(r"_ZN5snerf\d+sun_walk_ks_kernelILi(\d+)EEEv", k[".name"])
            if m:
                walk_ks[int(m.group(1))] = k
    return walk, walk_ks


def test_walk_kernels_exist_for_their_widths(walk_kernels):
    walk, walk_ks = walk_kernels
    assert sorted(walk) == [64, 256] and sorted(walk_ks) == [512], (sorted(walk), sorted(walk_ks))


@pytest.mark.parametrize("W", [64, 256, 512])
def test_walk_kernel_code_object_contract(walk_kernels, W):
    """No scratch, 256 threads, at most 512 registers, and no spilled vector register at W = 64 / 256 (at most 16 for the wave-pair kernel).  The trunk of
    W = 256 uses all 256 VGPRs, so any VGPR-only value that lives across the persistent tile loop shows up here (csrc/kernels.hip store_softplus)."""
    k = (walk_kernels[1] if W == 512 else walk_kernels[0])[W]
    print(f"  W={W}: vgpr {k['.vgpr_count']} agpr {k.get('.agpr_count')} sgpr {k['.sgpr_count']} spills v{k['.vgpr_spill_count']} s{k['.sgpr_spill_count']} "
          f"scratch {k['.private_segment_fixed_size']}")
    assert k[".private_segment_fixed_size"] == 0, (W, "uses scratch")
    assert k[".max_flat_workgroup_size"] == 256
    assert k[".vgpr_count"] <= 512
    if W == 512:
        assert k[".vgpr_spill_count"] <= 16, (W, k[".vgpr_spill_count"])
    else:
        assert k[".vgpr_spill_count"] == 0, (W, k[".vgpr_spill_count"])


def test_walk_ops_register_without_a_gpu():
    import season_nerf_amd as sn
    ns = sn.ops.load()
    for op in ["sun_walk_fwd", "composite_sun_walk"]:
        assert hasattr(ns, op), op
    s = str(torch.ops.season_nerf.sun_walk_fwd.default._schema)
    assert "Tensor suns" in s and "Tensor? classes" in s and s.endswith("-> Tensor[]"), s
    s = str(torch.ops.season_nerf.composite_sun_walk.default._schema)
    assert "Tensor solar_vis" in s and "Tensor? deltas=None" in s, s
    for f in ["component_render_sun_walk", "render_sun_season_walk"]:
        assert callable(getattr(sn, f))
    if not torch.cuda.is_available():
        z = torch.zeros
        with pytest.raises((RuntimeError, NotImplementedError)):          # no CPU backend: the ops never compute on the host
            torch.ops.season_nerf.composite_sun_walk(z(2, 3), z(2, 3), z(4), z(2, 4, 1), z(2, 4, 3), z(2, 4, 4, 3), z(1, 2, 4, 1), z(1, 3), z(1, 4), 2)
