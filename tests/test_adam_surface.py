"""The optimizer's kernel templates (csrc/dd_adam.h) without a GPU: the instantiations the two libraries hold and their registers, read
from the code objects' metadata."""
from _surface import kernel_resources

BUDGET = 48      # vector registers the conv backward's one-wave-per-SIMD kernels leave of a SIMD's 512 (csrc/dd_adam.h, include/dd_adamw.h)


def instantiations(kernel):
    """{(DEV, DECAY): metadata} of ``kernel<DEV, DECAY>``: without DECAY in the main library, with it in libdd_adamw.so."""
    from driving_dirty_amd import build
    tag = f"{len(kernel)}{kernel}I"
    found = {}
    for decay, lib in ((False, build.LIB), (True, build.OPTIMIZER_EXTENSIONS["adamw"].lib)):
        ks = [k for k in kernel_resources().kernels(lib) if tag in k[".name"]]
        assert len(ks) == 2, (lib, [k[".name"] for k in ks])
        for dev in (False, True):
            found[dev, decay], = [k for k in ks if f"{tag}Lb{int(dev)}ELb{int(decay)}E" in k[".name"]]
    return found


def no_scratch_no_spills(k):
    return k[".private_segment_fixed_size"] == 0 and k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0


def test_the_four_streaming_instantiations_have_one_register_count_within_the_budget():
    ks = instantiations("adam_kernel")
    assert len(ks) == 4
    counts = {form: k[".vgpr_count"] + k.get(".agpr_count", 0) for form, k in ks.items()}
    assert len(set(counts.values())) == 1 and max(counts.values()) <= BUDGET, counts
    for form, k in ks.items():
        assert no_scratch_no_spills(k), (form, k)


def test_the_four_table_instantiations_use_no_scratch():
    ks = instantiations("adam_multi_kernel")
    assert len(ks) == 4
    for form, k in ks.items():
        assert no_scratch_no_spills(k), (form, k)
