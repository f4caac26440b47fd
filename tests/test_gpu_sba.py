"""GPU bundle adjustment (ekf_sba_*) against the numpy oracle tests/sba_oracle.py."""
import numpy as np
import pytest

import sba_oracle as so
import sba_scene as sc

pytestmark = pytest.mark.gpu

# (free nodes, points): launch-bound to factor-bound
SIZES = [(1, 40), (11, 300), (59, 2000), (299, 8000)]
NITER = 10
COST_RTOL = 1e-9          # per-iteration costs
STATE_TOL = 1e-8          # final nodes and points, times the scene scale


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def gpu_system(pkg, scene, **caps):
    ba = pkg.BundleAdjuster(scene["camera"], capacity_nodes=caps.get("nodes", len(scene["nodes"])),
                            capacity_points=caps.get("points", len(scene["points"])),
                            capacity_projections=caps.get("projections", len(scene["node"])))
    ba.add_nodes(scene["nodes"])
    ba.add_points(scene["points"])
    ba.add_projections(scene["node"], scene["point"], scene["uv"])
    return ba


@pytest.mark.parametrize("nfree,npts", SIZES)
def test_run_matches_oracle(pkg, nfree, npts):
    scene = sc.make_scene(nfree, npts, seed=nfree)
    ref = sc.oracle_system(scene)
    ba = gpu_system(pkg, scene)
    assert ba.counts() == (len(ref.trans), len(ref.points), ref.nprojs)
    c0, r0 = ba.cost()
    assert np.isclose(c0, ref.calc_cost(), rtol=COST_RTOL, atol=0)
    assert np.isclose(r0, ref.calc_rms_cost(), rtol=COST_RTOL, atol=0)
    it = ba.run(NITER, 1e-4)
    it_ref = ref.do_sba(NITER, 1e-4)
    log, log_ref = ba.log(), np.array(ref.log, dtype=np.float64).reshape(-1, 5)
    assert it == it_ref and log.shape == log_ref.shape
    assert np.array_equal(log[:, 3], log_ref[:, 3])                  # accept / reject sequence
    assert np.array_equal(log[:, 2], log_ref[:, 2])                  # lambda: the same sequence of exact halvings / doublings
    np.testing.assert_allclose(log[:, :2], log_ref[:, :2], rtol=COST_RTOL, atol=0)
    tol = STATE_TOL * scene["scale"]
    np.testing.assert_allclose(ba.nodes(), ref.pose7(), rtol=0, atol=tol)
    np.testing.assert_allclose(ba.points(), np.array(ref.points), rtol=0, atol=tol)
    assert ba.rms_cost() < r0


def test_two_runs_are_bitwise_identical(pkg):
    scene = sc.make_scene(59, 2000, seed=3)
    out = []
    for _ in range(2):
        ba = gpu_system(pkg, scene)
        ba.run(NITER, 1e-4)
        out.append((ba.nodes(), ba.points(), ba.log()))
        ba.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


def test_non_positive_pivot_is_reported_and_keeps_the_state(pkg):
    # node 1 at the origin sees a point at the origin: p_c.z = 0, its Jacobians are NaN (not deviation 1)
    scene = sc.make_scene(3, 40, seed=5, lonely_node=False)
    scene["nodes"][1, :3] = 0.0
    scene["points"][0] = 0.0
    scene["node"] = np.concatenate([scene["node"], [1]]).astype(np.int32)
    scene["point"] = np.concatenate([scene["point"], [0]]).astype(np.int32)
    scene["uv"] = np.vstack([scene["uv"], [[300.0, 200.0]]])
    ba = gpu_system(pkg, scene)
    n0, p0 = ba.nodes(), ba.points()
    with pytest.raises(pkg.EkfError) as ei:
        ba.run(NITER, 1e-4)
    assert ei.value.status == 5                                      # EKF_ERR_NUMERIC
    assert np.array_equal(ba.nodes(), n0) and np.array_equal(ba.points(), p0)


def test_capacity_and_argument_errors(pkg):
    scene = sc.make_scene(2, 40, seed=7)
    ba = pkg.BundleAdjuster(scene["camera"], capacity_nodes=3, capacity_points=40, capacity_projections=10)
    ba.add_nodes(scene["nodes"])
    with pytest.raises(pkg.EkfError) as ei:
        ba.add_nodes(scene["nodes"][:1])
    assert ei.value.status == 2
    ba.add_points(scene["points"])
    with pytest.raises(pkg.EkfError) as ei:
        ba.add_points(scene["points"][:1])
    assert ei.value.status == 2
    with pytest.raises(pkg.EkfError) as ei:
        ba.add_projections(scene["node"][:11], scene["point"][:11], scene["uv"][:11])
    assert ei.value.status == 2 and ba.counts()[2] == 0             # all or nothing
    with pytest.raises(pkg.EkfError) as ei:
        ba.add_projections([3], [0], [[1.0, 2.0]])
    assert ei.value.status == 1
    with pytest.raises(pkg.EkfError) as ei:
        ba.add_projections([0], [0], [[np.nan, 2.0]])
    assert ei.value.status == 1
    # duplicates: the same keypoint is a no-op, another keypoint is rejected
    assert ba.add_projections([1, 1, 1], [0, 0, 0], [[5.0, 6.0], [5.0, 6.0], [7.0, 6.0]]) == 1
    assert ba.counts()[2] == 1


def test_empty_problem_and_single_node(pkg):
    scene = sc.make_scene(1, 40, seed=9)
    ba = pkg.BundleAdjuster(scene["camera"], capacity_nodes=2, capacity_points=40, capacity_projections=100)
    assert ba.run(10, 1e-4) == -1
    ba.add_nodes(scene["nodes"][:1])
    ba.add_points(scene["points"])
    sel = scene["node"] == 0
    ba.add_projections(scene["node"][sel], scene["point"][sel], scene["uv"][sel])
    n0, p0 = ba.nodes(), ba.points()
    assert ba.run(10, 1e-4) == 0                                      # no free node: converged at iteration 0
    assert np.array_equal(ba.nodes(), n0) and np.array_equal(ba.points(), p0)


def test_sba_add_driver_matches_oracle(pkg, tmp_path):
    """The driver over the three files, GPU and oracle, with a record every 10 nodes (RMS wrapper on the way)."""
    from ekf_monoslam_amd import formats
    scene = sc.make_scene(21, 300, seed=11, noise_px=0.0)
    cam = scene["camera"]
    # row 0 is a real point, observed like the others (deviation 3: the reference never adds it); the last row is
    # all zero and is not added
    table = np.zeros((len(scene["points"]) + 1, 12), np.float32)
    table[:-1, :3] = scene["points"]
    table[:-1, 3] = table[:-1, 7] = table[:-1, 11] = 1e-4
    assert (scene["point"] == 0).any()
    recs = []
    for i, pose in enumerate(scene["nodes"]):
        sel = scene["node"] == i
        prj = np.stack([scene["point"][sel], np.floor(scene["uv"][sel, 0]), np.floor(scene["uv"][sel, 1])], 1)
        recs.append(formats.pose_record(i, pose, prj if len(prj) else None))
    (tmp_path / "points.txt").write_text(formats.format_eigen(table) + "\n")
    (tmp_path / "nodes_and_prjcts.txt").write_text("".join(recs))
    (tmp_path / "cams_cov.txt").write_text("".join(formats.camera_cov_record(np.eye(7)) for _ in recs))
    out, nodes, ids = pkg.sba_add(str(tmp_path / "points.txt"), str(tmp_path / "nodes_and_prjcts.txt"),
                                  str(tmp_path / "cams_cov.txt"), camera=cam, points_out=str(tmp_path / "Points_Out.txt"),
                                  nodes_out=str(tmp_path / "Nodes_Out.txt"))
    ref, rows, ref_ids = so.sba_add(formats.read_points(str(tmp_path / "points.txt")),
                                    formats.read_pose_records(str(tmp_path / "nodes_and_prjcts.txt")), camera=cam)
    assert ids == ref_ids == list(range(len(scene["nodes"])))
    assert rows == list(range(len(scene["points"])))                # row 0 added, the zero row not
    assert not out[-1].any()
    tol = 1e-6 * scene["scale"]
    np.testing.assert_allclose(out[rows], np.array(ref.points), rtol=0, atol=tol)
    np.testing.assert_allclose(nodes, ref.pose7(), rtol=0, atol=tol)
    back = formats.read_points_out(str(tmp_path / "Points_Out.txt"))
    np.testing.assert_allclose(back, np.array(ref.points), rtol=1e-5, atol=1e-5 * scene["scale"])
    assert formats.read_nodes_out(str(tmp_path / "Nodes_Out.txt"))[0] == ids


def test_cost_rejects_a_bad_dist_with_its_own_message(pkg):
    scene = sc.make_scene(3, 40, seed=5, lonely_node=False)
    ba = gpu_system(pkg, scene)
    with pytest.raises(pkg.EkfError) as ei:
        ba.cost(0.0)
    assert ei.value.status == 1 and "dist" in str(ei.value)


def test_filter_stream_keyframes_to_sba_add(pkg, tmp_path):
    """End to end: an fp64 filter stream (the image stream of test_gpu_end_update.py) with conversions to XYZ forced
    by shrinking the inverse-depth rows of Sigma, a key frame every 3 frames (pose, 7 x 7 block, keyframeProjections()),
    the three files written with `formats` and the table of ekf_export_points_table; sba.sba_add on the GPU against the
    oracle driver on the same files."""
    import ekf_oracle as o
    import test_gpu_end_update as ge
    from ekf_monoslam_amd import formats
    cfg = ge._stream_config()
    ref = o.StructuredFilter(o.Config.kinect(), np.float64)
    g = pkg.VSlamFilter(cfg, capacity_features=128, dtype=np.float64)
    g.setDt(1.0 / 30.0)
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    world = ge._stream_world()
    g.setFrame(ge._stream_frame(world, 0))
    g.findNewFeatures(-1)
    records, covs, nproj = [], [], 0
    for f in range(1, 19):
        ge._device_frame(g, ge._stream_frame(world, f), False)
        # force conversions: D Sigma D with D = 1e-4 on the 6 rows of up to 4 inverse-depth features (stays PSD)
        pos, cod = g.featureLayout()
        S = g.getFullSigma()
        for i in [i for i in range(len(cod)) if cod[i] == 0][:4]:
            p = int(pos[i])
            S[p:p + 6, :] *= 1e-4
            S[:, p:p + 6] *= 1e-4
        g.setSigmaBlock(S)
        g.convert2XYZ_ifLinearAll()
        if f % 3 == 0:
            mu = g.getFullState()
            prj = g.keyframeProjections()
            nproj += int(prj[0, 0] != 0) * len(prj)
            records.append(formats.pose_record(f, mu[:7], None if prj[0, 0] == 0 else prj))
            covs.append(formats.camera_cov_record(g.getSigmaBlock(0, 0, 7, 7)))
    table = g.getPointsTable()
    g.close()
    assert nproj >= 20, nproj
    formats.write_points(str(tmp_path / "points.txt"), table)
    (tmp_path / "nodes_and_prjcts.txt").write_text("".join(records))
    (tmp_path / "cams_cov.txt").write_text("".join(covs))
    cam = (cfg["fx"], cfg["fy"], cfg["u0"], cfg["v0"])
    files = [str(tmp_path / n) for n in ("points.txt", "nodes_and_prjcts.txt", "cams_cov.txt")]
    out, nodes, ids = pkg.sba_add(*files, camera=cam, every=3, points_out=str(tmp_path / "Points_Out.txt"),
                                  nodes_out=str(tmp_path / "Nodes_Out.txt"))
    pts, recs = formats.read_points(files[0]), formats.read_pose_records(files[1])
    ref_sys, rows, ref_ids = so.sba_add(pts, recs, camera=cam, every=3)
    start, _, _ = so.sba_add(pts, recs, camera=cam, every=3, run=False)
    assert ids == ref_ids == [3 * (k + 1) for k in range(len(records))]
    scale = float(np.abs(pts[rows, :3]).max())
    err_p = float(np.abs(out[rows] - np.array(ref_sys.points)).max())
    err_n = float(np.abs(nodes - ref_sys.pose7()).max())
    print("filter stream -> sba_add: %d nodes, %d points, %d projections; rms %.4g -> %.4g; max |diff| nodes %.3g "
          "points %.3g (scale %.3g)" % (len(ids), len(rows), ref_sys.nprojs, start.calc_rms_cost(),
                                         ref_sys.calc_rms_cost(), err_n, err_p, scale))
    assert err_p <= 1e-8 * scale and err_n <= 1e-8 * scale
    assert ref_sys.calc_rms_cost() <= start.calc_rms_cost()
    ba_rms = pkg.BundleAdjuster(cam, capacity_nodes=len(ids), capacity_points=len(rows),
                                capacity_projections=max(ref_sys.nprojs, 1))
    ba_rms.add_nodes(nodes)
    ba_rms.add_points(out[rows])
    for ni, (_, _, prj) in enumerate(recs):
        sel = [(rows.index(int(r)), float(u), float(v)) for r, u, v in prj if (r, u, v) != (0, 0, 0) and int(r) in rows]
        if sel:
            s_ = np.array(sel)
            ba_rms.add_projections(np.full(len(sel), ni), s_[:, 0].astype(np.int32), s_[:, 1:])
    assert ba_rms.rms_cost() <= start.calc_rms_cost()
