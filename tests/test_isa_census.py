"""Code-object checks for the census matching cost, beside test_isa_sba_pcg.py: k_plane_sweep and
k_sweep_volume, whose body gained a template parameter, keep the registers and LDS of §15.2 and §19.3, and none of the five
sweep and descriptor kernels uses scratch or spills.  CPU only."""
from test_isa_sba_pcg import code_object, kernel_metadata  # noqa: F401  (the fixture)

# symbol needle -> (VGPRs, LDS bytes) the kernel must keep; None: recorded in §20.2, not held
KERNELS = {
    "13k_plane_sweepE": (80, 7104),
    "14k_sweep_volumeE": (72, 7104),
    "20k_plane_sweep_censusE": (None, 7104),
    "21k_sweep_volume_censusE": (None, 7104),
    "8k_censusE": (None, 880),
}


def test_sweep_kernels_keep_their_registers_and_none_uses_scratch(code_object):  # noqa: F811
    meta = kernel_metadata(code_object)
    for needle, (vgprs, lds) in KERNELS.items():
        names = [n for n in meta if needle in n]
        assert len(names) == 1, (needle, names)
        m = meta[names[0]]
        print(needle, "vgpr", m["vgpr_count"], "sgpr", m["sgpr_count"], "lds", m["group_segment_fixed_size"])
        assert m["private_segment_fixed_size"] == 0, f"{names[0]} uses {m['private_segment_fixed_size']} bytes of scratch"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
        assert m["group_segment_fixed_size"] == lds
        if vgprs is not None:
            assert m["vgpr_count"] == vgprs, (needle, m["vgpr_count"])
