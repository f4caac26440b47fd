"""Code-object checks for the device weld, in the manner of test_isa_speckle.py: each of the new kernels
occurs once (k_mesh_vertices once with and once without normals), uses no scratch and spills no register, its LDS is what
§24.2 states (the two rows of k_mesh_edges's scan: 2 x 256 words), its registers are printed for §24.2, and every fusion,
ray-cast and colour kernel still occurs once under its own name.  Metadata only.  CPU only."""
from test_isa_sba_pcg import code_object, kernel_metadata  # noqa: F401  (the fixture)

# symbol needle -> LDS bytes
KERNELS = {
    "12k_mesh_cellsE": 0,
    "12k_mesh_edgesE": 2048,
    "15k_mesh_verticesILb0EE": 0,
    "15k_mesh_verticesILb1EE": 0,
    "12k_mesh_facesE": 0,
}
OLD = ("16k_tsdf_integrateE", "12k_tsdf_countE", "11k_tsdf_scanE", "11k_tsdf_emitE", "11k_tsdf_meanE", "14k_tsdf_raycastE",
       "13k_bgr_to_greyE", "23k_tsdf_integrate_colourE", "22k_tsdf_colour_verticesE", "21k_tsdf_raycast_colourE")


def test_mesh_kernels_use_no_scratch_and_spill_nothing(code_object):  # noqa: F811
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
