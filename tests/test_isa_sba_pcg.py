"""Code-object checks for the PCG solver of the bundle adjuster, beside test_isa_invariants.py: none of
its kernels uses scratch, and k_sba_point -- the Schur kernel both solvers share -- still compiles to the instructions
it had before the solver was added (tests/golden/sba_isa.json holds their digest).  CPU only."""
import hashlib
import json
import os
import re
import subprocess
import tempfile

import pytest

import test_isa_invariants as isa

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
GOLDEN = os.path.join(isa.ROOT, "tests", "golden", "sba_isa.json")
NEW_KERNELS = ["k_sba_pairs_blk", "k_sba_diag_blk", "k_sba_blk_inv", "k_sba_cg_mv", "k_sba_cg_stepILb1E",
               "k_sba_cg_stepILb0E", "k_sba_cg_dirILb1E", "k_sba_cg_dirILb0E", "k_sba_cg_end"]


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(isa.LIB):
        import __graft_entry__ as g
        g.build()
    if not (os.path.exists(isa.OBJDUMP) and os.path.exists(READELF)):
        pytest.skip("llvm tools missing")
    with tempfile.NamedTemporaryFile(suffix=".co", delete=False) as f:
        f.write(isa._code_object())
    yield f.name
    os.unlink(f.name)


def kernel_metadata(path):
    """{kernel symbol: {field: int}} from the AMDGPU metadata note."""
    out = subprocess.run([READELF, "--notes", path], capture_output=True, text=True, check=True).stdout
    meta = {}
    for blk in out.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(v) for k, v in re.findall(r"\.(\w+):\s+(\d+)\s*$", blk, flags=re.M)}
    return meta


def instruction_digest(path, needle):
    """sha256 over the instructions of the one kernel whose symbol contains `needle`, addresses stripped."""
    out = subprocess.run([isa.OBJDUMP, "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
    bodies = re.findall(r"^[0-9a-f]+ <([^>]*%s[^>]*)>:\n(.*?)\n\n" % re.escape(needle), out, flags=re.S | re.M)
    assert len(bodies) == 1, [b[0] for b in bodies]
    lines = [re.sub(r"\s*//.*$", "", l).strip() for l in bodies[0][1].splitlines()]
    lines = [l for l in lines if l and not l.startswith("s_nop") and not l.startswith("s_code_end")]
    return hashlib.sha256("\n".join(lines).encode()).hexdigest(), len(lines)


def test_new_kernels_use_no_scratch(code_object):
    meta = kernel_metadata(code_object)
    for needle in NEW_KERNELS:
        names = [n for n in meta if needle in n]
        assert len(names) == 1, (needle, names)
        m = meta[names[0]]
        print(needle, "vgpr", m["vgpr_count"], "sgpr", m["sgpr_count"], "lds", m["group_segment_fixed_size"])
        assert m["private_segment_fixed_size"] == 0, f"{names[0]} uses {m['private_segment_fixed_size']} bytes of scratch"
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0


def test_k_sba_point_is_unchanged(code_object):
    want = json.load(open(GOLDEN))["k_sba_point"]
    digest, n = instruction_digest(code_object, "k_sba_pointE")
    assert (digest, n) == (want["sha256"], want["instructions"])
    # the dense destination of the shared pair summation keeps its registers
    meta = kernel_metadata(code_object)
    pairs = [m for name, m in meta.items() if "k_sba_pairsE" in name]
    assert len(pairs) == 1 and pairs[0]["vgpr_count"] == json.load(open(GOLDEN))["k_sba_pairs"]["vgpr_count"]
