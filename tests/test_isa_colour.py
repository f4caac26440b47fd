"""Code-object checks for the four colour kernels of the dense chain, in the manner of test_isa_fusion.py: the
gfx950 code object holds each of them once, and none of them uses scratch or spills.  CPU only."""
import test_isa_sba_pcg as base
from test_isa_sba_pcg import code_object  # noqa: F401  (fixture)

KERNELS = ["k_bgr_to_greyE", "k_tsdf_integrate_colourE", "k_tsdf_colour_verticesE", "k_tsdf_raycast_colourE"]


def test_colour_kernels_exist_without_scratch(code_object):  # noqa: F811
    meta = base.kernel_metadata(code_object)
    for needle in KERNELS:
        names = [n for n in meta if needle in n]
        assert len(names) == 1, (needle, names)
        m = meta[names[0]]
        print(needle, "vgpr", m["vgpr_count"], "sgpr", m["sgpr_count"], "lds", m["group_segment_fixed_size"])
        assert m["private_segment_fixed_size"] == 0, f"{names[0]} uses {m['private_segment_fixed_size']} bytes of scratch"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0
