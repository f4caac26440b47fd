"""Code-object checks for the mesh-to-mesh distance, in the manner of test_isa_raster.py: each of the eight new
kernels occurs once, uses no scratch and spills no register (no kernel has a per-lane array), has the LDS §31.2 states, its
registers are printed for §31.2, and every raster, texture, simplification, smoothing, mesh, component, speckle and fusion kernel
still occurs once under its own name.  Metadata only.  CPU only."""
from test_isa_sba_pcg import code_object, kernel_metadata  # noqa: F401  (the fixture)
from test_isa_raster import KERNELS as RASTER
from test_isa_simplify import KERNELS as SIMPLIFY
from test_isa_smooth import KERNELS as SMOOTH, OLD
from test_isa_texture import KERNELS as TEXTURE

# symbol needle -> LDS bytes
KERNELS = {
    "10k_dist_boxE": 3072,
    "11k_dist_gridE": 3072,
    "12k_dist_countE": 0,
    "14k_dist_offsetsE": 2048,
    "11k_dist_fillE": 0,
    "12k_dist_queryE": 0,
    "12k_dist_statsE": 6144,
    "13k_dist_reduceE": 6144,
}


def test_distance_kernels_use_no_scratch_and_spill_nothing(code_object):  # noqa: F811
    meta = kernel_metadata(code_object)
    for needle, lds in KERNELS.items():
        names = [n for n in meta if needle in n]
        assert len(names) == 1, (needle, names)
        m = meta[names[0]]
        print(needle, "vgpr", m["vgpr_count"], "sgpr", m["sgpr_count"], "lds", m["group_segment_fixed_size"])
        assert m["private_segment_fixed_size"] == 0, f"{names[0]} uses {m['private_segment_fixed_size']} bytes of scratch"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
        assert m["group_segment_fixed_size"] == lds
    for needle in tuple(RASTER) + tuple(TEXTURE) + tuple(SIMPLIFY) + tuple(SMOOTH) + tuple(OLD):
        assert len([n for n in meta if needle in n]) == 1, needle
