"""CPU checks of the robust bundle-adjustment oracle (tests/sba_robust_oracle.py), the argument checks of the new
ekf_sba_* functions that run without a device, and the code-object figures DESIGN.md §11.6 records."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import sba_robust_oracle as ro
import sba_robust_scene as rs
import sba_scene as sc
import test_isa_invariants as isa

READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"
# k_sba_point in the parent commit's build: no scratch, 112 VGPRs
PARENT_POINT_PRIVATE_SEGMENT = 0


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def test_huber_weight_known_answers():
    # e = (3, 4), huber = 1: e2 = 25 > 1, c = 2 * 1 * 5 - 1 = 9, w = sqrt(9 / 25) = 0.6, weighted e = (1.8, 2.4), |e|^2 = 9
    e, e2 = ro.huber_weight(np.array([3.0, 4.0]), 1.0)
    np.testing.assert_allclose(e, [1.8, 2.4], rtol=1e-15)
    assert math.isclose(e2, 9.0, rel_tol=1e-15)
    # e2 <= b2 leaves e untouched (the boundary included: the test is e2 > b2)
    for h in (5.0, 6.0, 0.0):
        e, e2 = ro.huber_weight(np.array([3.0, 4.0]), h)
        assert e.tolist() == [3.0, 4.0] and e2 == 25.0
    # the weighted squared error is 2 h |e| - h^2: linear in |e|
    e, e2 = ro.huber_weight(np.array([0.0, 30.0]), 2.0)
    assert math.isclose(e2, 2 * 2 * 30 - 4, rel_tol=1e-15)


def test_point_behind_the_camera_has_zero_error_with_and_without_huber():
    w2i = np.hstack([np.eye(3), np.zeros((3, 1))])
    for h in (0.0, 2.0):
        for X in ([0.3, 0.2, -1.0], [0.3, 0.2, 0.0]):
            e, e2 = ro.proj_error(w2i, np.array(X), np.array([100.0, 50.0]), h)
            assert not e.any() and e2 == 0.0


def _robust_copy(scene, huber=0.0):
    s = ro.RobustSysSBA(scene["camera"], huber)
    for p in scene["nodes"]:
        s.add_node(p)
    for x in scene["points"]:
        s.add_point(x)
    for ni, pi, m in zip(scene["node"], scene["point"], scene["uv"]):
        s.add_proj(int(ni), int(pi), m)
    return s


def test_huber_zero_and_all_valid_is_the_plain_oracle_bit_for_bit():
    scene = sc.make_scene(11, 300, seed=1)
    a, b = sc.oracle_system(scene), _robust_copy(scene)
    assert a.nprojs == b.nprojs
    assert a.calc_cost() == b.calc_cost() and a.calc_rms_cost() == b.calc_rms_cost()
    assert a.do_sba(10, 1e-4) == b.do_sba(10, 1e-4)
    assert a.log == b.log and len(a.log) > 0
    assert a.pose7().tobytes() == b.pose7().tobytes()
    assert np.array(a.points).tobytes() == np.array(b.points).tobytes()


def test_pruned_oracle_equals_an_oracle_built_without_those_projections():
    scene = rs.make_robust_scene(5, 120, seed=2)
    s = rs.oracle_system(scene, 2.0)
    s.do_sba(5, 1e-4)
    n = s.count_bad(10.0)
    assert n > 0 and s.remove_bad(10.0) == n and s.count_bad(10.0) == 0
    node, point, uv, valid = s.projections()
    assert len(node) == len(scene["node"]) and int((~valid).sum()) == n      # the slots are still there
    s.reduce_tracks()
    node, point, uv, valid = s.projections()
    assert valid.all() and len(node) < len(scene["node"])
    # afresh: the same current state, only the surviving projections, in the same loop order
    f = ro.RobustSysSBA(scene["camera"], 2.0)
    for p in s.pose7():
        f.add_node(p)
    f.qrot = [q.copy() for q in s.qrot]                                   # add_node renormalises: keep the exact state
    for x in s.points:
        f.add_point(x)
    for ni, pi, m in zip(node, point, uv):
        f.add_proj(int(ni), int(pi), m)
    assert s.calc_cost() == f.calc_cost()
    assert s.do_sba(5, 1e-4) == f.do_sba(5, 1e-4)
    assert s.log == f.log and len(s.log) > 0
    assert s.pose7().tobytes() == f.pose7().tobytes()
    assert np.array(s.points).tobytes() == np.array(f.points).tobytes()


def test_invalid_projections_contribute_nothing_and_block_repeats():
    scene = rs.make_robust_scene(4, 60, seed=3)
    s = rs.oracle_system(scene, 2.0)
    pi = 0
    nodes = sorted(s.tracks[pi])
    for ni in nodes:
        s.valid[pi][ni] = False
    kept = rs.oracle_system(scene, 2.0, keep=scene["point"] != pi)
    assert s.calc_cost() == kept.calc_cost() and s.calc_avg_error() == kept.calc_avg_error()
    A1, B1, _, _ = s.setup_sparse_sys(1e-4)
    A2, B2, _, _ = kept.setup_sparse_sys(1e-4)
    assert np.array_equal(A1, A2) and np.array_equal(B1, B2)
    assert s.nprojs == kept.nprojs + len(nodes)                              # stored, not valid, projections
    assert not s.add_proj(nodes[0], pi, (1.0, 2.0)) and s.nprojs == kept.nprojs + len(nodes)
    x0 = s.points[pi].copy()
    s.do_sba(3, 1e-4)
    assert np.array_equal(s.points[pi], x0)                                  # deviation 1: the point is left alone
    assert np.isfinite(np.array(s.points)).all() and np.isfinite(s.pose7()).all()


def test_reduce_tracks_counts_short_and_empty_tracks():
    s = ro.RobustSysSBA(sc.CAMERA)
    for _ in range(3):
        s.add_node([0, 0, 0, 1, 0, 0, 0])
    for z in (5.0, 6.0, 7.0, 8.0):
        s.add_point([0, 0, z])
    for ni in range(3):
        s.add_proj(ni, 0, (320.0, 240.0))
        s.add_proj(ni, 1, (320.0, 240.0))
    s.add_proj(0, 2, (320.0, 240.0))                                         # a single-projection track; point 3 has none
    s.valid[1][0] = s.valid[1][1] = False                                    # point 1 keeps one valid projection
    assert s.reduce_tracks() == 3                                            # points 1, 2 and the empty 3
    assert [len(t) for t in s.tracks] == [3, 0, 0, 0]
    assert math.isnan(ro.RobustSysSBA(sc.CAMERA).calc_avg_error())


def test_new_abi_checks_without_a_device(pkg):
    lib = pkg.load_library()
    n, d = C.c_int(), C.c_double()
    assert lib.ekf_sba_set_huber(None, 1.0) == 1
    assert lib.ekf_sba_get_huber(None, C.byref(d)) == 1
    assert lib.ekf_sba_count_bad(None, 10.0, C.byref(n)) == 1
    assert lib.ekf_sba_remove_bad(None, 10.0, C.byref(n)) == 1
    assert lib.ekf_sba_reduce_tracks(None, C.byref(n)) == 1
    assert lib.ekf_sba_num_bad_points(None, C.byref(n)) == 1
    assert lib.ekf_sba_avg_error(None, C.byref(d)) == 1
    assert lib.ekf_sba_get_projections(None, 0, None, None, None, None, C.byref(n)) == 1
    for name in ("huber", "count_bad", "remove_bad", "reduce_tracks", "num_bad_points", "avg_error", "projections"):
        assert hasattr(pkg.BundleAdjuster, name), name


def _kernel_metadata():
    """{kernel name: {field: int}} from the AMDGPU metadata note of the built library's gfx950 code object."""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(isa._code_object())
        f.flush()
        out = subprocess.run([READELF, "--notes", f.name], capture_output=True, text=True, check=True).stdout
    kernels, cur = {}, {}
    for line in out.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(\S+)\s*$", line)
        if not m:
            continue
        key, val = m.groups()
        if key == "name" and val.startswith("_Z"):
            cur.setdefault("name", val)
        elif key in ("private_segment_fixed_size", "vgpr_count", "vgpr_spill_count", "wavefront_size"):
            cur[key] = int(val)
        if key == "wavefront_size":                                          # the last key of a kernel's record
            kernels[cur.get("name", "?")] = cur
            cur = {}
    return kernels


def test_sba_kernels_use_no_more_scratch_than_the_parent():
    if not (os.path.exists(isa.LIB) and os.path.exists(READELF)):
        pytest.skip("library or llvm-readelf missing")
    meta = _kernel_metadata()

    def one(needle):
        hit = [v for k, v in meta.items() if needle in k]
        assert len(hit) == 1, (needle, [k for k in meta if needle in k])
        return hit[0]

    point = one("k_sba_pointE")
    print("k_sba_point: private segment %d B, %d VGPRs" % (point["private_segment_fixed_size"], point["vgpr_count"]))
    assert point["private_segment_fixed_size"] <= PARENT_POINT_PRIVATE_SEGMENT
    assert point["vgpr_spill_count"] == 0
    assert point["vgpr_count"] <= 128                                        # four waves per SIMD, as the parent's 112
    for needle in ("k_sba_flag_badE", "k_sba_statsE"):
        k = one(needle)
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, (needle, k)
