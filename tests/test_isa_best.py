"""Code-object checks for the best-K source selection, beside test_isa_census.py, which keeps holding the
figures of the existing sweep kernels: none of the four new kernels uses scratch or spills a register (the sorted list of
the selection is indexed by compile-time constants alone), and their registers and LDS are printed for §21.2.  CPU only."""
from test_isa_sba_pcg import code_object, kernel_metadata  # noqa: F401  (the fixture)

KERNELS = ("18k_plane_sweep_bestE", "25k_plane_sweep_best_censusE", "19k_sweep_volume_bestE", "26k_sweep_volume_best_censusE")
OLD = ("13k_plane_sweepE", "14k_sweep_volumeE", "20k_plane_sweep_censusE", "21k_sweep_volume_censusE")


def test_best_kernels_use_no_scratch_and_spill_nothing(code_object):  # noqa: F811
    meta = kernel_metadata(code_object)
    for needle in KERNELS:
        names = [n for n in meta if needle in n]
        assert len(names) == 1, (needle, names)
        m = meta[names[0]]
        print(needle, "vgpr", m["vgpr_count"], "sgpr", m["sgpr_count"], "lds", m["group_segment_fixed_size"])
        assert m["private_segment_fixed_size"] == 0, f"{names[0]} uses {m['private_segment_fixed_size']} bytes of scratch"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
        assert 0 < m["group_segment_fixed_size"] <= 64 * 1024
    for needle in OLD:                                              # the new names hide inside none of the old needles
        assert len([n for n in meta if needle in n]) == 1, needle
