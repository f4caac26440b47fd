"""Code-object checks for the mesh smoothing, in the manner of test_isa_components.py: each of the six new
kernels occurs once, uses no scratch and spills no register (the lists are ordered in place in global memory: no kernel has a
per-lane array), its LDS is what §26.2 states (k_smooth_offsets: the two rows of the scan; the others none), its registers are
printed for §26.2, and every mesh, component, speckle and fusion kernel still occurs once under its own name.  Metadata only.
CPU only."""
from test_isa_sba_pcg import code_object, kernel_metadata  # noqa: F401  (the fixture)

# symbol needle -> LDS bytes
KERNELS = {
    "14k_smooth_countE": 0,
    "16k_smooth_offsetsE": 2048,
    "13k_smooth_fillE": 0,
    "14k_smooth_listsE": 0,
    "13k_smooth_stepE": 0,
    "16k_smooth_normalsE": 0,
}
OLD = ("12k_mesh_cellsE", "12k_mesh_edgesE", "15k_mesh_verticesILb0EE", "15k_mesh_verticesILb1EE", "12k_mesh_facesE",
       "11k_comp_initE", "12k_comp_unionE", "12k_comp_countE", "14k_comp_largestE", "12k_comp_flagsE", "15k_comp_verticesE",
       "12k_comp_facesE",
       "15k_speckle_labelE", "15k_speckle_mergeE", "15k_speckle_countE", "15k_speckle_applyE",
       "16k_tsdf_integrateE", "12k_tsdf_countE", "11k_tsdf_scanE", "11k_tsdf_emitE", "11k_tsdf_meanE", "14k_tsdf_raycastE",
       "13k_bgr_to_greyE", "23k_tsdf_integrate_colourE", "22k_tsdf_colour_verticesE", "21k_tsdf_raycast_colourE")


def test_smooth_kernels_use_no_scratch_and_spill_nothing(code_object):  # noqa: F811
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
