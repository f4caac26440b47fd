"""Code-object checks for the speckle filter, beside test_isa_unique.py, which keeps holding the figures of
the kernels it stands behind: each of the four new kernels occurs once, uses no scratch and spills no register, its LDS is
what §23.2 states (the tile's planes and forest: 2 x 512 words; the tile's counters, keys and runs: 3 x 512 words), its
registers are printed for §23.2, and every dense kernel still occurs once under its own name.  Metadata only.  CPU only."""
from test_isa_sba_pcg import code_object, kernel_metadata  # noqa: F401  (the fixture)

# symbol needle -> LDS bytes
KERNELS = {
    "15k_speckle_labelE": 4096,
    "15k_speckle_mergeE": 0,
    "15k_speckle_countE": 6144,
    "15k_speckle_applyE": 0,
}
OLD = ("13k_plane_sweepE", "20k_plane_sweep_censusE", "18k_plane_sweep_bestE", "25k_plane_sweep_best_censusE", "12k_sgm_winnerE",
       "21k_depth_filter_pointsE", "14k_sweep_volumeE", "21k_sweep_volume_censusE", "19k_sweep_volume_bestE",
       "26k_sweep_volume_best_censusE", "20k_plane_sweep_uniqueE", "27k_plane_sweep_census_uniqueE", "25k_plane_sweep_best_uniqueE",
       "32k_plane_sweep_best_census_uniqueE", "19k_sgm_winner_uniqueE", "21k_depth_filter_uniqueE", "8k_censusE")


def test_speckle_kernels_use_no_scratch_and_spill_nothing(code_object):  # noqa: F811
    meta = kernel_metadata(code_object)
    for needle, lds in KERNELS.items():
        names = [n for n in meta if needle in n]
        assert len(names) == 1, (needle, names)
        m = meta[names[0]]
        print(needle, "vgpr", m["vgpr_count"], "sgpr", m["sgpr_count"], "lds", m["group_segment_fixed_size"])
        assert m["private_segment_fixed_size"] == 0, f"{names[0]} uses {m['private_segment_fixed_size']} bytes of scratch"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
        assert m["group_segment_fixed_size"] == lds
    for needle in OLD:
        assert len([n for n in meta if needle in n]) == 1, needle
