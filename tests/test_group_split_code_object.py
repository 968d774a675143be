"""Register contract of the split per-ray kernel (csrc/kernels_group.hip), read from the code-object metadata of the shipped library: no GPU, no compile
beyond the library's own build, no instruction text.

The kernel keeps a layer's input (16 Frags at W = 256), a ring of requested weight pairs and the pre-requested pairs of its next layers in registers, all
indexed statically after unrolling.  A rolled loop over one of those arrays, or one live value too many, would show as scratch or as spilled registers -
and a latency chain that goes through scratch is what the kernel exists to avoid."""
import importlib.util
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _guards():
    """tests/test_isa_guards.py: the one reader of the library's fat binary and of its code-object metadata."""
    spec = importlib.util.spec_from_file_location("snerf_isa_guards", os.path.join(REPO, "tests", "test_isa_guards.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_split_group_kernel_uses_no_scratch_and_spills_nothing():
    spec = importlib.util.spec_from_file_location("snerf_build", os.path.join(REPO, "season_nerf_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build()
    found, g = {}, _guards()
    for elf in g._device_code_objects(b.LIB):
        for k in g._kernel_metadata(elf):
            m = re.match(r"_ZN5snerf\d+mlp_group_split_kernelILi(\d+)EEEv", k[".name"])
            if m:
                found[int(m.group(1))] = k
    assert sorted(found) == [64, 256], sorted(found)
    for W, k in found.items():
        print(f"  W={W}: vgpr {k['.vgpr_count']} agpr {k.get('.agpr_count')} sgpr {k['.sgpr_count']} spills v{k['.vgpr_spill_count']} s{k['.sgpr_spill_count']} "
              f"scratch {k['.private_segment_fixed_size']} lds {k['.group_segment_fixed_size']}")
        assert k[".private_segment_fixed_size"] == 0, (W, "uses scratch")
        assert k[".vgpr_spill_count"] == 0 and k[".sgpr_spill_count"] == 0, (W, k[".vgpr_spill_count"], k[".sgpr_spill_count"])
        # one wave per SIMD, four waves per workgroup.  The kernel is laid out for 267 (W = 256) / 132 (W = 64) registers: G_T2's input, one ring of eight weight
        # pairs, two blocks' accumulators and epilogue values.  The bound leaves a compiler release some room and still fails when a second layer's ring or
        # input becomes live beside them (64 / 128 registers at W = 256) - the state in which hipcc parked registers while the kernel was written.
        assert k[".max_flat_workgroup_size"] == 256
        assert k[".vgpr_count"] <= {256: 300, 64: 160}[W], (W, k[".vgpr_count"])
        assert k[".group_segment_fixed_size"] == 0        # the two activation buffers are dynamic LDS, sized by the launcher
