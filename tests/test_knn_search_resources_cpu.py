"""The compile-time resources of csrc/knn_search.hip, as the shipped flags build it: the twelve instantiations of the tile
kernel (list lengths 8, 16 and 32, each without / with the inner-dimension tail, each with exclusion by index and by label)
stay inside 256 VGPRs - two workgroups of four waves per CU for the lists of 8 and 16 keys, one for the 32-key lists, which
alone take half of a wave's registers - and no kernel of the file uses scratch memory.  The 16-key form sits at 256 VGPRs
exactly: one more live value costs it its second workgroup.  Both policies share ONE merge kernel per list length."""
import re

from kernel_resources import needs_hipcc, read_source, resource_usage

POLICIES = ("ByIndex", "ByLabel")


@needs_hipcc
def test_search_kernels_of_both_policies_keep_their_workgroups_per_cu_and_use_no_scratch():
    usage = resource_usage("knn_search.hip")
    source = read_source("knn_search.hip")
    declared = re.findall(r"\b(\w+_kernel)\(const", source)
    assert declared == ["knn_search_kernel", "knn_search_merge_kernel"], declared      # ONE tile kernel, ONE merge kernel
    assert source.count("__global__") == 2 and "asm" not in source
    assert "__launch_bounds__(ENGINE_THREADS, KCAP <= 16 ? 2 : 1)" in source
    tile = {n: u for n, u in usage.items() if re.search(r"knn_search_kernelILi(8|16|32)ELb[01]E", n)}
    merge = {n: u for n, u in usage.items() if re.search(r"knn_search_merge_kernelILi(8|16|32)E", n)}
    # every list length without / with the inner-dimension tail under either policy, and one merge kernel per list length
    assert sorted(re.search(r"ILi(\d+)ELb([01])ENS\d_\d+(By\w+?)E", n).groups() for n in tile) == \
        sorted((str(k), t, p) for k in (8, 16, 32) for t in "01" for p in POLICIES), sorted(tile)
    assert sorted(re.search(r"ILi(\d+)E", n).group(1) for n in merge) == ["16", "32", "8"], sorted(merge)
    assert len(tile) == 12 and len(merge) == 3 and len(usage) == 15, sorted(usage)     # every __global__ kernel of the file
    for n, u in usage.items():
        print(n, u)
        assert u["scratch"] == 0, (n, u)
    for n, u in tile.items():
        kcap = int(re.search(r"ILi(\d+)E", n).group(1))
        assert u["vgprs"] <= 256 and u["occupancy"] >= (2 if kcap <= 16 else 1), (n, u)
