"""Code-object checks for the mesh simplification, in the manner of test_isa_smooth.py: each of the nine new
kernels occurs once, uses no scratch and spills no register (the lists are ordered in place in global memory: no kernel has a
per-lane array), its LDS is what §28.2 states (k_simp_offsets: the two rows of the scan; k_simp_flags: those and one counter;
the others none), its registers are printed for §28.2, and every smoothing, mesh, component, speckle and fusion kernel still
occurs once under its own name.  Metadata only.  CPU only."""
from test_isa_sba_pcg import code_object, kernel_metadata  # noqa: F401  (the fixture)
from test_isa_smooth import KERNELS as SMOOTH, OLD

# symbol needle -> LDS bytes
KERNELS = {
    "12k_simp_cellsE": 0,
    "12k_simp_countE": 0,
    "14k_simp_offsetsE": 2048,
    "11k_simp_fillE": 0,
    "12k_simp_listsE": 0,
    "12k_simp_flagsE": 2052,
    "15k_simp_verticesE": 0,
    "12k_simp_facesE": 0,
    "10k_simp_mapE": 0,
}


def test_simplify_kernels_use_no_scratch_and_spill_nothing(code_object):  # noqa: F811
    meta = kernel_metadata(code_object)
    for needle, lds in KERNELS.items():
        names = [n for n in meta if needle in n]
        assert len(names) == 1, (needle, names)
        m = meta[names[0]]
        print(needle, "vgpr", m["vgpr_count"], "sgpr", m["sgpr_count"], "lds", m["group_segment_fixed_size"])
        assert m["private_segment_fixed_size"] == 0, f"{names[0]} uses {m['private_segment_fixed_size']} bytes of scratch"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
        assert m["group_segment_fixed_size"] == lds
    for needle in tuple(SMOOTH) + tuple(OLD):
        assert len([n for n in meta if needle in n]) == 1, needle
