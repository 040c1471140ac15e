"""The compile-time resources of csrc/retrieval.hip, as the shipped flags build it: the four instantiations of the tile
kernel (without / with the inner-dimension tail, every column / other groups only) keep two workgroups of four waves on a CU
(at most 256 VGPRs, occupancy >= 2, two workgroups inside the 160 KiB of LDS) and no kernel of the file uses scratch memory -
a threshold and two counts per lane and row, and with groups two label registers and a second column array, must not cost
registers the accumulator tile needs."""
import re

from kernel_resources import needs_hipcc, read_source, resource_usage

POLICIES = {"AllColumns": 1, "OtherGroups": 2}                             # policy -> per-column arrays through LDS


@needs_hipcc
def test_tile_kernels_of_both_policies_keep_two_workgroups_per_cu_and_use_no_scratch():
    usage = resource_usage("retrieval.hip")
    source = read_source("retrieval.hip")
    declared = re.findall(r"\b(\w+_kernel)\(const", source)
    assert declared == ["retrieval_weights_kernel", "retrieval_positives_kernel", "retrieval_kernel", "retrieval_merge_kernel"], declared
    assert source.count("__global__") == 4 and "asm" not in source
    assert "atomic" not in source.split("#include")[1]                     # no atomics of any kind in the code
    assert "__launch_bounds__(ENGINE_THREADS, 2)" in source
    assert "dense_pipeline_early<EV_DEFAULT, KTAIL>" in source and "launch_sweep(" in source and "choose_chunks(" in source
    # staging slabs + [2][ARRAYS][128] floats, ARRAYS from the policy; that two workgroups fit in a CU's LDS under both is
    # checked where ENGINE_LDS_FLOATS is known, by the compiler (the build of `usage` above went through it)
    assert "(ENGINE_LDS_FLOATS + 2 * Excl::ARRAYS * TB) * sizeof(float)" in source
    assert "static_assert(2 * LDS_BYTES<AllColumns> <= 160 * 1024 && 2 * LDS_BYTES<OtherGroups> <= 160 * 1024," in source
    for policy, arrays in POLICIES.items():
        assert re.search(r"struct %s \{[^}]*static constexpr int ARRAYS = %d;" % (policy, arrays), source), policy
    tile = {n: u for n, u in usage.items() if "retrieval_kernel" in n}
    # the tile kernel without / with the inner-dimension tail under either policy
    assert sorted(re.search(r"ILb([01])ENS\d_\d+(\w+?)EEE", n).groups() for n in tile) == \
        sorted((t, p) for t in "01" for p in POLICIES), sorted(tile)
    assert len(tile) == 4 and len(usage) == 7 and all(any(k in n for n in usage) for k in declared), sorted(usage)   # every __global__ kernel
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
    for n, u in tile.items():
        assert u["vgprs"] <= 256 and u["occupancy"] >= 2, (n, u)
