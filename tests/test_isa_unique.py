"""Code-object checks for the runner-up cost and the uniqueness test, beside test_isa_census.py and
test_isa_best.py, which keep holding the figures of the existing sweep kernels: none of the six new kernels uses scratch or
spills a register (the four keys of a pixel are indexed by compile-time constants alone), their registers and LDS are printed
for §22.2, and every kernel they stand beside still occurs once under its own name.  CPU only."""
from test_isa_sba_pcg import code_object, kernel_metadata  # noqa: F401  (the fixture)

# symbol needle -> LDS bytes (those of the kernel's twin)
KERNELS = {
    "20k_plane_sweep_uniqueE": 7104,
    "27k_plane_sweep_census_uniqueE": 7104,
    "25k_plane_sweep_best_uniqueE": 28416,
    "32k_plane_sweep_best_census_uniqueE": 28416,
    "19k_sgm_winner_uniqueE": 0,
    "21k_depth_filter_uniqueE": 0,
}
OLD = ("13k_plane_sweepE", "20k_plane_sweep_censusE", "18k_plane_sweep_bestE", "25k_plane_sweep_best_censusE", "12k_sgm_winnerE",
       "21k_depth_filter_pointsE", "14k_sweep_volumeE", "21k_sweep_volume_censusE", "19k_sweep_volume_bestE",
       "26k_sweep_volume_best_censusE")


def test_unique_kernels_use_no_scratch_and_spill_nothing(code_object):  # noqa: F811
    meta = kernel_metadata(code_object)
    for needle, lds in KERNELS.items():
        names = [n for n in meta if needle in n]
        assert len(names) == 1, (needle, names)
        m = meta[names[0]]
        print(needle, "vgpr", m["vgpr_count"], "sgpr", m["sgpr_count"], "lds", m["group_segment_fixed_size"])
        assert m["private_segment_fixed_size"] == 0, f"{names[0]} uses {m['private_segment_fixed_size']} bytes of scratch"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
        assert m["group_segment_fixed_size"] == lds
    for needle in OLD:                                              # the new names hide inside none of the old needles
        assert len([n for n in meta if needle in n]) == 1, needle
