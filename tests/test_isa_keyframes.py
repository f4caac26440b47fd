"""Code-object checks for the key-frame selector, in the manner of test_isa_sba_pcg.py: the gfx950 code
object holds k_keyframe_probe for both dtypes and k_keyframe_snapshot, none of them uses scratch, and k_sba_point still
compiles to the instructions recorded in tests/golden/sba_isa.json.  CPU only."""
import json

import test_isa_sba_pcg as base
from test_isa_sba_pcg import code_object  # noqa: F401  (fixture)

KERNELS = ["k_keyframe_probeIfE", "k_keyframe_probeIdE", "k_keyframe_snapshotE"]


def test_keyframe_kernels_exist_without_scratch(code_object):  # noqa: F811
    meta = base.kernel_metadata(code_object)
    for needle in KERNELS:
        names = [n for n in meta if needle in n]
        assert len(names) == 1, (needle, names)
        m = meta[names[0]]
        print(needle, "vgpr", m["vgpr_count"], "sgpr", m["sgpr_count"], "lds", m["group_segment_fixed_size"])
        assert m["private_segment_fixed_size"] == 0, f"{names[0]} uses {m['private_segment_fixed_size']} bytes of scratch"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0


def test_k_sba_point_metadata_is_unchanged(code_object):  # noqa: F811
    want = json.load(open(base.GOLDEN))
    digest, n = base.instruction_digest(code_object, "k_sba_pointE")
    assert (digest, n) == (want["k_sba_point"]["sha256"], want["k_sba_point"]["instructions"])
    meta = base.kernel_metadata(code_object)
    pairs = [m for name, m in meta.items() if "k_sba_pairsE" in name]
    assert len(pairs) == 1 and pairs[0]["vgpr_count"] == want["k_sba_pairs"]["vgpr_count"]
