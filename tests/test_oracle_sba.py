"""CPU checks of the bundle-adjustment oracle (tests/sba_oracle.py), the Points_Out / Nodes_Out formats and the
ekf_sba_* argument checks that run without a device."""
import ctypes as C
import io

import numpy as np
import pytest

import sba_oracle as so
import sba_scene as sc


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _local_rot(q, d):
    """The camera update's rotation increment (sba.cpp:1450-1458)."""
    qr = np.array([np.sqrt(1.0 - d @ d), *d])
    q2 = so.quat_mul(q, qr)
    return q2 / np.linalg.norm(q2)


def test_jacobians_match_central_differences():
    rng = np.random.default_rng(0)
    cam = sc.CAMERA
    t = np.array([0.1, -0.2, 0.3])
    q = so.norm_rot(np.array([0.9, 0.1, -0.2, 0.05]))
    X = t + so.quat_rot(q) @ np.array([0.3, -0.2, 4.0])
    kp = np.array([300.0, 250.0])

    def err(t_, q_, X_):
        w2n, w2i, _ = so.node_mats(t_, q_, cam)
        return so.proj_error(w2i, X_, kp)[0]

    w2n, _, dR = so.node_mats(t, q, cam)
    jacc, jacp = so.proj_jacobians(w2n, dR, t, X, cam)
    h = 1e-6
    for k in range(3):
        e = np.eye(3)[k] * h
        np.testing.assert_allclose((err(t + e, q, X) - err(t - e, q, X)) / (2 * h), jacc[:, k], rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose((err(t, _local_rot(q, e), X) - err(t, _local_rot(q, -e), X)) / (2 * h),
                                   jacc[:, 3 + k], rtol=1e-5, atol=1e-3)
        np.testing.assert_allclose((err(t, q, X + e) - err(t, q, X - e)) / (2 * h), jacp[:, k], rtol=1e-5, atol=1e-4)
    del rng


def test_lm_reaches_the_pixel_noise():
    scene = sc.make_scene(11, 300, seed=1, noise_px=0.5)
    s = sc.oracle_system(scene)
    rms0 = s.calc_rms_cost()
    assert rms0 > 5.0
    it = s.do_sba(20, 1e-4)
    assert it > 0 and s.calc_rms_cost() < 0.7                  # 2-D noise of 0.5 px per axis, less the fitted dof
    np.testing.assert_array_equal(s.trans[0], scene["nodes"][0, :3])   # node 0 is fixed


def test_node_zero_is_fixed_and_free_nodes_move():
    scene = sc.make_scene(3, 60, seed=2)
    s = sc.oracle_system(scene)
    start = s.pose7().copy()
    s.do_sba(5, 1e-4)
    assert np.array_equal(s.pose7()[0], start[0])
    assert not np.array_equal(s.pose7()[1], start[1])


def test_point_behind_the_camera_keeps_its_hessian_terms():
    scene = sc.make_scene(3, 60, seed=4)
    s = sc.oracle_system(scene)
    m = s._mats()
    behind = len(s.points) - 1                                   # the scene's last points lie behind every camera
    ni = sorted(s.tracks[behind])[0]
    e, c = so.proj_error(m[ni][1], s.points[behind], s.tracks[behind][ni])
    assert c == 0.0 and not e.any()
    jacc, jacp = so.proj_jacobians(m[ni][0], m[ni][2], s.trans[ni], s.points[behind], s.camera)
    assert np.abs(jacp.T @ jacp).max() > 0 and np.abs(jacc.T @ jacc).max() > 0
    # the point's Schur terms are in A: dropping the point changes the system
    A1, _, _, _ = s.setup_sparse_sys(1e-4)
    s.tracks[behind] = {}
    A2, _, _, _ = s.setup_sparse_sys(1e-4)
    assert not np.array_equal(A1, A2)


def test_duplicate_projection_rule():
    s = so.SysSBA()
    s.add_node([0, 0, 0, 1, 0, 0, 0])
    s.add_point([0, 0, 5])
    assert s.add_proj(0, 0, (10.0, 20.0))
    assert s.add_proj(0, 0, (10.0, 20.0))                        # same keypoint: a no-op
    assert not s.add_proj(0, 0, (11.0, 20.0))                    # another keypoint: rejected, the first stays
    assert s.nprojs == 1 and np.array_equal(s.tracks[0][0], [10.0, 20.0])


def test_single_node_and_converged_start_and_empty_problem():
    assert so.SysSBA().do_sba(10, 1e-4) == -1
    scene = sc.make_scene(1, 40, seed=6, noise_px=0.0)
    one = so.SysSBA(scene["camera"])
    one.add_node(scene["nodes"][0])
    for x in scene["points"]:
        one.add_point(x)
    for ni, pi, m in zip(scene["node"], scene["point"], scene["uv"]):
        if ni == 0:
            one.add_proj(0, int(pi), m)
    pts = [p.copy() for p in one.points]
    assert one.do_sba(10, 1e-4) == 0                             # no free node: |x|^2 = 0 at iteration 0
    assert all(np.array_equal(a, b) for a, b in zip(pts, one.points))
    # exact start, exact keypoints (points in front): |x|^2 < 1e-16 stops at iteration 0
    s = so.SysSBA(scene["camera"])
    for p in scene["true_nodes"]:
        s.add_node(p)
    for x in scene["true_points"][:-2]:
        s.add_point(x)
    m = s._mats()
    for pi, x in enumerate(s.points):
        for ni in range(2):
            p1 = m[ni][1] @ np.append(x, 1.0)
            s.add_proj(ni, pi, p1[:2] / p1[2])
    assert s.do_sba(10, 1e-4) == 0 and s.log == []


def test_projectionless_free_node_gets_an_identity_block():
    scene = sc.make_scene(4, 60, seed=8)                         # the last node has no projection
    s = sc.oracle_system(scene)
    A, B, _, _ = s.setup_sparse_sys(1e-4)
    c = 6 * (len(s.trans) - 2)
    np.testing.assert_array_equal(A[c:c + 6, c:c + 6], np.eye(6))
    assert not A[c:c + 6, :c].any() and not B[c:c + 6].any()
    last = s.pose7()[-1].copy()
    s.do_sba(5, 1e-4)
    np.testing.assert_array_equal(s.pose7()[-1, :3], last[:3])


def _files(table, records):
    from ekf_monoslam_amd import formats
    return formats.read_points(io.StringIO(formats.format_eigen(table))), formats.read_pose_records(
        io.StringIO("".join(formats.pose_record(pid, pose, prj) for pid, pose, prj in records)))


def test_driver_deviations(pkg):
    scene = sc.make_scene(1, 40, seed=10, noise_px=0.0)
    table = np.zeros((4, 12), np.float32)
    table[:3, :3] = scene["true_points"][:3]                     # row 0 is a real point; row 3 is all zero
    m = [so.node_mats(p[:3], so.norm_rot(p[3:]), scene["camera"])[1] for p in scene["true_nodes"]]
    prj = lambda n, r: [r, *np.floor((m[n] @ np.append(table[r, :3], 1))[:2] / (m[n] @ np.append(table[r, :3], 1))[2])]  # noqa: E731
    records = [(0, scene["true_nodes"][0], np.array([prj(0, 0), prj(0, 1), [3, 100, 100]])),
               (1, scene["true_nodes"][1], None),                 # "0  0  0": no projection
               (2, scene["true_nodes"][1], np.array([prj(1, 0), prj(1, 2)]))]
    pts, recs = _files(table, records)
    assert [r[0] for r in recs] == [0, 1, 2] and recs[1][2].tolist() == [[0, 0, 0]]
    s, rows, ids = so.sba_add(pts, recs, camera=scene["camera"], every=0)
    assert ids == [0, 1, 2]                                      # P0 is a node id, not the end of the file
    assert rows == [0, 1, 2] and len(s.points) == 3              # row 0 added; the zero row 3 not; no duplicate last row
    assert sorted(s.tracks[0]) == [0, 2] and sorted(s.tracks[1]) == [0] and sorted(s.tracks[2]) == [2]
    assert s.nprojs == 4                                         # the 0 0 0 line and the zero-row projection are not projections


def test_points_and_nodes_out_round_trip(pkg):
    from ekf_monoslam_amd import formats
    xyz = np.array([[1.5, -2.25, 3.0], [0.001, 12.5, -7.75]])
    b = io.StringIO()
    formats.write_points_out(b, xyz)
    assert b.getvalue().endswith("\n")
    np.testing.assert_array_equal(formats.read_points_out(io.StringIO(b.getvalue())), xyz)
    poses = np.array([[0.5, -1.0, 2.0, 1.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 0.5, 0.5, 0.5, 0.5]])
    b = io.StringIO()
    formats.write_nodes_out(b, [0, 7], poses)
    assert b.getvalue().startswith("P0\n") and "\nP7\n" in b.getvalue()
    ids, back = formats.read_nodes_out(io.StringIO(b.getvalue()))
    assert ids == [0, 7]
    np.testing.assert_allclose(back, poses, rtol=1e-6)


def test_abi_checks_without_a_device(pkg):
    import torch
    lib = pkg.load_library()
    h = C.c_void_p()
    bad = pkg.sba.SbaCamera(-1.0, 500.0, 320.0, 240.0)
    assert lib.ekf_sba_create(C.byref(bad), 10, 10, 10, 0, C.byref(h)) == 1       # bad arguments first
    assert b"bad argument" in lib.ekf_sba_last_error(None)
    good = pkg.sba.SbaCamera(*sc.CAMERA)
    assert lib.ekf_sba_create(C.byref(good), 2000, 10, 10, 0, C.byref(h)) == 1    # beyond 1024 nodes
    assert lib.ekf_sba_create(C.byref(good), 10, 0, 10, 0, C.byref(h)) == 1
    assert lib.ekf_sba_run(None, 1, 1e-4, None) == 1
    assert lib.ekf_sba_add_nodes(None, 1, None) == 1
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(pkg.EkfError) as ei:
        pkg.BundleAdjuster(sc.CAMERA)
    assert ei.value.status == 3 and "no HIP device" in str(ei.value)


def test_point4sba_rows(pkg):
    """vslamRansac.cpp:1319-1336: in innovation and XYZ-coded only, (int) truncation of the centre, row 0 rewritten
    while its first entry is 0, the 640 x 480 bound on every later row, `0 0 0` when nothing qualifies."""
    from ekf_monoslam_amd import formats
    ri = [4, 5, 6, 7, 8, 9, 10]
    inn = [1, 0, 1, 1, 1, 1, 1]
    cod = [1, 1, 0, 1, 1, 1, 1]
    cen = [[10.7, 20.2], [1, 1], [2, 2], [700.0, 5.0], [30.9, 479.9], [-0.5, 3.0], [639.99, 480.0]]
    rows = formats.point4sba_rows(ri, inn, cod, cen)
    assert rows.tolist() == [[4, 10, 20], [8, 30, 479], [9, 0, 3]]
    # the first qualifying row is outside the bound: row 0 takes it anyway
    assert formats.point4sba_rows([3, 2], [1, 1], [1, 1], [[900, 900], [5, 6]]).tolist() == [[3, 900, 900], [2, 5, 6]]
    # a real_index 0 in row 0 is overwritten by the next qualifying feature (`if (Point4sba(0) == 0)`)
    assert formats.point4sba_rows([0, 2], [1, 1], [1, 1], [[1, 1], [5, 6]]).tolist() == [[2, 5, 6]]
    assert formats.point4sba_rows([1], [1], [0], [[1, 1]]).tolist() == [[0, 0, 0]]
