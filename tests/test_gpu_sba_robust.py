"""Robust GPU bundle adjustment (pseudo-Huber cost, validity flags, pruning) against the numpy oracle
tests/sba_robust_oracle.py.  Tolerances are those of tests/test_gpu_sba.py."""
import copy
import functools
import math

import numpy as np
import pytest

import sba_robust_oracle as ro
import sba_robust_scene as rs
import sba_scene as sc

pytestmark = pytest.mark.gpu

SIZES = [(1, 40), (11, 300), (59, 2000)]
NITER = 10
COST_RTOL = 1e-9          # per-iteration costs (tests/test_gpu_sba.py)
STATE_TOL = 1e-8          # final nodes and points, times the scene scale (tests/test_gpu_sba.py)
HUBER = 2.0               # pixels
DIST = 10.0               # pruning threshold: 0.5 px noise, outliers of 30 px and more (weighted: |e|^2 >= 116)
MARGIN = 1e-6             # no oracle e^2 may lie this close (relative) to DIST^2, or a count could flip on rounding


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def gpu_system(pkg, scene, huber=0.0, keep=None):
    ba = pkg.BundleAdjuster(scene["camera"], capacity_nodes=len(scene["nodes"]), capacity_points=len(scene["points"]),
                            capacity_projections=len(scene["node"]))
    ba.add_nodes(scene["nodes"])
    ba.add_points(scene["points"])
    sel = slice(None) if keep is None else keep
    ba.add_projections(scene["node"][sel], scene["point"][sel], scene["uv"][sel])
    ba.huber = huber
    return ba


@functools.lru_cache(maxsize=None)
def _scene(nfree, npts):
    return rs.make_robust_scene(nfree, npts, seed=nfree)


@functools.lru_cache(maxsize=None)
def _oracle_after_run(nfree, npts, huber):
    """(oracle after do_sba(NITER), its iteration count); callers deep-copy before they change it."""
    s = rs.oracle_system(_scene(nfree, npts), huber)
    it = s.do_sba(NITER, 1e-4)
    return s, it


def assert_run_matches(ba, it, ref, it_ref, scene):
    log, log_ref = ba.log(), np.array(ref.log, dtype=np.float64).reshape(-1, 5)
    assert it == it_ref and log.shape == log_ref.shape
    assert np.array_equal(log[:, 3], log_ref[:, 3])                  # accept / reject sequence
    assert np.array_equal(log[:, 2], log_ref[:, 2])                  # lambda
    np.testing.assert_allclose(log[:, :2], log_ref[:, :2], rtol=COST_RTOL, atol=0)
    assert_state_matches(ba, ref, scene)


def assert_state_matches(ba, ref, scene):
    tol = STATE_TOL * scene["scale"]
    np.testing.assert_allclose(ba.nodes(), ref.pose7(), rtol=0, atol=tol)
    np.testing.assert_allclose(ba.points(), np.array(ref.points), rtol=0, atol=tol)


def assert_clear_of_threshold(ref, dist):
    e = ref.errors()
    gap = float(np.min(np.abs(e / (dist * dist) - 1.0)))
    assert gap > MARGIN, "the scene or dist is wrong: an oracle e^2 lies within %.3g of dist^2" % gap


# 1 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfree,npts", SIZES)
def test_huber_run_matches_oracle(pkg, nfree, npts):
    scene = _scene(nfree, npts)
    assert scene["outlier"].sum() == round(0.05 * len(scene["node"]))
    ba = gpu_system(pkg, scene, HUBER)
    assert ba.huber == HUBER
    start = rs.oracle_system(scene, HUBER)
    c0, r0 = ba.cost()
    assert np.isclose(c0, start.calc_cost(), rtol=COST_RTOL, atol=0)
    assert np.isclose(r0, start.calc_rms_cost(), rtol=COST_RTOL, atol=0)
    plain = rs.oracle_system(scene, 0.0).calc_cost()
    assert start.calc_cost() < 0.5 * plain                           # the weight bites on this scene
    it = ba.run(NITER, 1e-4)
    ref, it_ref = _oracle_after_run(nfree, npts, HUBER)
    assert_run_matches(ba, it, ref, it_ref, scene)


# 2 ---------------------------------------------------------------------------------------------------------
def test_a_huber_width_that_never_bites_changes_no_bit(pkg):
    scene = _scene(11, 300)
    out = []
    for h in (0.0, 1e6):
        ba = gpu_system(pkg, scene, h)
        c = ba.cost()
        ba.run(NITER, 1e-4)
        out.append((np.array(c), ba.nodes(), ba.points(), ba.log(), np.array([ba.avg_error()])))
        ba.close()
    assert len(out[0][3]) > 0
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


# 3 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfree,npts", SIZES)
def test_counts_and_flags_are_exact(pkg, nfree, npts):
    scene = _scene(nfree, npts)
    ref = copy.deepcopy(_oracle_after_run(nfree, npts, HUBER)[0])
    assert_clear_of_threshold(ref, DIST)
    ba = gpu_system(pkg, scene, HUBER)
    ba.run(NITER, 1e-4)
    nstored = len(scene["node"])
    assert ba.counts()[2] == nstored == ref.nprojs
    assert ba.num_bad_points() == ref.num_bad_points()
    assert math.isclose(ba.avg_error(), ref.calc_avg_error(), rel_tol=1e-12)
    nbad = ref.count_bad(DIST)
    assert nbad > 0 and ba.count_bad(DIST) == nbad
    assert ba.projections()[3].all()                                  # counting marks nothing
    assert ba.remove_bad(DIST) == ref.remove_bad(DIST) == nbad
    assert ba.count_bad(DIST) == ref.count_bad(DIST) == 0
    for got, want in zip(ba.projections(), ref.projections()):
        assert np.array_equal(got, want)
    assert ba.counts()[2] == nstored                                  # the slots stay until reduce_tracks
    assert ba.num_bad_points() == ref.num_bad_points()
    assert math.isclose(ba.avg_error(), ref.calc_avg_error(), rel_tol=1e-12)
    c, r = ba.cost()
    assert np.isclose(c, ref.calc_cost(), rtol=COST_RTOL, atol=0) and np.isclose(r, ref.calc_rms_cost(), rtol=COST_RTOL)
    # an invalid projection still blocks a repeat of its pair
    node, point, uv, valid = ba.projections()
    k = int(np.flatnonzero(~valid)[0])
    assert ba.add_projections([node[k]], [point[k]], [uv[k] + 1.0]) == 0
    assert ba.reduce_tracks() == ref.reduce_tracks()
    assert ba.counts()[2] == ref.nprojs < nstored
    for got, want in zip(ba.projections(), ref.projections()):
        assert np.array_equal(got, want)
    assert ba.projections()[3].all()


# 4 ---------------------------------------------------------------------------------------------------------
def test_pruned_equals_rebuilt_bit_for_bit(pkg):
    """Pruning at the start state (whose own weighted error stays below the threshold), so that the second handle can
    be given the identical state through the same add calls."""
    scene = _scene(11, 300)
    a = gpu_system(pkg, scene, HUBER)
    removed = a.remove_bad(DIST)
    assert removed > 0
    a.reduce_tracks()
    node, point, uv, valid = a.projections()
    assert valid.all() and len(node) < len(scene["node"])
    stored = set(zip(node.tolist(), point.tolist()))
    keep = np.array([(int(n), int(p)) in stored for n, p in zip(scene["node"], scene["point"])])
    assert keep.sum() == len(node)
    b = gpu_system(pkg, scene, HUBER, keep=keep)
    for x, y in zip(a.projections(), b.projections()):
        assert np.array_equal(x, y)
    ca, cb = a.cost(), b.cost()
    ia, ib = a.run(NITER, 1e-4), b.run(NITER, 1e-4)
    assert ia == ib and ia > 0 and ca == cb
    for x, y in ((a.nodes(), b.nodes()), (a.points(), b.points()), (a.log(), b.log())):
        assert x.tobytes() == y.tobytes()
    assert a.avg_error() == b.avg_error()


# 5 ---------------------------------------------------------------------------------------------------------
def _three_ways(make, run, prune):
    out = {}
    for name, h, p in (("plain", 0.0, False), ("huber", HUBER, False), ("huber+prune", HUBER, True)):
        s = make(h)
        run(s)
        if p:
            prune(s)
        out[name] = s
    return out


def test_robust_cost_and_pruning_recover_the_poses(pkg):
    """make_robust_scene(11, 300, seed=11): 5 % of the projections are 30-80 px outliers.  The oracle alone, on the
    CPU, 10 iterations from the perturbed start (RMS camera-centre error against true_nodes, world units; the start
    is 0.0192):
        huber = 0                                             0.0695
        huber = 2                                             0.0480
        huber = 2, remove_bad(10) + reduce_tracks + 10 more   0.0141
    The GPU must match the oracle in all three and show the same ordering; no ratio is asserted."""
    scene = _scene(11, 300)

    def prune_ref(s):
        assert_clear_of_threshold(s, DIST)
        assert s.remove_bad(DIST) > 0
        s.reduce_tracks()
        s.do_sba(NITER, 1e-4)

    def prune_gpu(ba):
        assert ba.remove_bad(DIST) > 0
        ba.reduce_tracks()
        ba.run(NITER, 1e-4)

    refs = _three_ways(lambda h: copy.deepcopy(_oracle_after_run(11, 300, h)[0]), lambda s: None, prune_ref)
    gpus = _three_ways(lambda h: gpu_system(pkg, scene, h), lambda ba: ba.run(NITER, 1e-4), prune_gpu)
    err_ref = {k: rs.pose_error(v.pose7(), scene) for k, v in refs.items()}
    err_gpu = {k: rs.pose_error(v.nodes(), scene) for k, v in gpus.items()}
    print("pose error, oracle:", err_ref, "GPU:", err_gpu)
    for k in refs:
        assert_state_matches(gpus[k], refs[k], scene)
        assert gpus[k].counts()[2] == refs[k].nprojs
    assert err_ref["huber+prune"] < err_ref["plain"]                 # what the oracle showed
    assert err_gpu["huber+prune"] < err_gpu["plain"]


# 6 ---------------------------------------------------------------------------------------------------------
def test_all_invalid_point_and_node_are_left_alone(pkg):
    """Deviations 1 and 2 of DESIGN.md §11.6.  Every keypoint of node 3 and of point 5 is moved by 200 px; remove_bad
    at the start state then strips both of every projection.  (18 points: the scene then has none behind the cameras,
    whose zero error no threshold removes.)"""
    scene = copy.deepcopy(_scene(4, 18))
    lost_node, lost_point = 3, 5
    sel = (scene["node"] == lost_node) | (scene["point"] == lost_point)
    scene["uv"][sel] += 200.0
    ref = rs.oracle_system(scene, 0.0)
    assert_clear_of_threshold(ref, 100.0)
    ba = gpu_system(pkg, scene, 0.0)
    assert ba.remove_bad(100.0) == ref.remove_bad(100.0)
    node, point, _, valid = ba.projections()
    assert not valid[node == lost_node].any() and not valid[point == lost_point].any()
    assert valid[(node != lost_node) & (point != lost_point)].sum() > 40
    for got, want in zip(ba.projections(), ref.projections()):
        assert np.array_equal(got, want)
    n0, p0 = ba.nodes(), ba.points()
    it, it_ref = ba.run(NITER, 1e-4), ref.do_sba(NITER, 1e-4)
    assert it > 0
    assert_run_matches(ba, it, ref, it_ref, scene)
    n1, p1 = ba.nodes(), ba.points()
    assert np.isfinite(n1).all() and np.isfinite(p1).all() and np.isfinite(ba.log()).all()
    assert p1[lost_point].tobytes() == p0[lost_point].tobytes()       # deviation 1
    assert n1[lost_node, :3].tobytes() == n0[lost_node, :3].tobytes()  # deviation 2: a zero step
    np.testing.assert_allclose(n1[lost_node, 3:], n0[lost_node, 3:], rtol=0, atol=4e-16)   # renormalised only
    assert not np.array_equal(n1[1], n0[1])


# 7 ---------------------------------------------------------------------------------------------------------
def _write_files(scene, tmp_path):
    from ekf_monoslam_amd import formats
    table = np.zeros((len(scene["points"]) + 1, 12), np.float32)
    table[:-1, :3] = scene["points"]
    table[:-1, 3] = table[:-1, 7] = table[:-1, 11] = 1e-4
    recs = []
    for i, pose in enumerate(scene["nodes"]):
        sel = scene["node"] == i
        prj = np.stack([scene["point"][sel], np.floor(scene["uv"][sel, 0]), np.floor(scene["uv"][sel, 1])], 1)
        recs.append(formats.pose_record(i, pose, prj if len(prj) else None))
    (tmp_path / "points.txt").write_text(formats.format_eigen(table) + "\n")
    (tmp_path / "nodes_and_prjcts.txt").write_text("".join(recs))
    (tmp_path / "cams_cov.txt").write_text("".join(formats.camera_cov_record(np.eye(7)) for _ in recs))
    return [str(tmp_path / n) for n in ("points.txt", "nodes_and_prjcts.txt", "cams_cov.txt")]


def test_sba_add_driver_with_huber_and_pruning_matches_oracle(pkg, tmp_path):
    from ekf_monoslam_amd import formats
    scene = rs.make_robust_scene(21, 300, seed=11)
    files = _write_files(scene, tmp_path)
    out, nodes, ids = pkg.sba_add(*files, camera=scene["camera"], huber=HUBER, prune_dist=DIST)
    ref, rows, ref_ids = ro.sba_add(formats.read_points(files[0]), formats.read_pose_records(files[1]),
                                    camera=scene["camera"], huber=HUBER, prune_dist=DIST)
    assert ids == ref_ids
    assert ref.nprojs < len(scene["node"])                           # the pruning did something
    tol = 1e-6 * scene["scale"]                                      # test_sba_add_driver_matches_oracle's bound
    np.testing.assert_allclose(out[rows], np.array(ref.points), rtol=0, atol=tol)
    np.testing.assert_allclose(nodes, ref.pose7(), rtol=0, atol=tol)


def test_sba_add_defaults_are_the_plain_driver_bit_for_bit(pkg, tmp_path):
    """The call of test_sba_add_driver_matches_oracle against the driver loop as it was before `huber` and
    `prune_dist` existed, replayed here over BundleAdjuster.rms_wrapper."""
    from ekf_monoslam_amd import formats
    scene = sc.make_scene(21, 300, seed=11, noise_px=0.0)
    files = _write_files(scene, tmp_path)
    out, nodes, ids = pkg.sba_add(*files, camera=scene["camera"])
    table, records = formats.read_points(files[0]), formats.read_pose_records(files[1])
    rows = [i for i in range(table.shape[0]) if table[i, :3].any()]
    row_of = {r: k for k, r in enumerate(rows)}
    ba = pkg.BundleAdjuster(scene["camera"], capacity_nodes=len(records), capacity_points=len(rows),
                            capacity_projections=sum(len(r[2]) for r in records))
    ba.add_points(table[rows, :3].astype(np.float64))
    for pid, pose, prj in records:
        ni = ba.add_nodes(np.asarray(pose, dtype=np.float32).astype(np.float64).reshape(1, 7))
        sel = [(row_of[int(ri)], float(int(u)), float(int(v))) for ri, u, v in np.asarray(prj).reshape(-1, 3)
               if not (ri == 0 and u == 0 and v == 0) and int(ri) in row_of]
        if sel:
            s = np.array(sel)
            ba.add_projections(np.full(len(sel), ni), s[:, 0].astype(np.int32), s[:, 1:])
        if (ni + 1) % 10 == 0:
            ba.rms_wrapper()
    ba.rms_wrapper()
    assert ba.huber == 0.0 and ba.projections()[3].all()
    assert out[rows].tobytes() == ba.points().tobytes() and nodes.tobytes() == ba.nodes().tobytes()


# 8 ---------------------------------------------------------------------------------------------------------
def test_huber_and_pruning_are_bitwise_reproducible(pkg):
    scene = _scene(59, 2000)
    out = []
    for _ in range(2):
        ba = gpu_system(pkg, scene, HUBER)
        ba.run(NITER, 1e-4)
        counts = [ba.remove_bad(DIST), ba.reduce_tracks(), ba.run(NITER, 1e-4), ba.num_bad_points()]
        out.append((ba.nodes(), ba.points(), ba.log(), np.array(counts), np.array([ba.avg_error()]), *ba.projections()))
        ba.close()
    assert out[0][3][0] > 0
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


def test_bad_huber_and_dist_are_rejected_with_their_own_messages(pkg):
    scene = _scene(1, 40)
    ba = gpu_system(pkg, scene, HUBER)
    before = (ba.nodes(), ba.points(), *ba.projections())
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(pkg.EkfError) as ei:
            ba.huber = bad
        assert ei.value.status == 1 and "huber" in str(ei.value)
    assert ba.huber == HUBER
    for call, name in ((ba.count_bad, "count_bad"), (ba.remove_bad, "remove_bad")):
        for bad in (0.0, -3.0, float("nan")):
            with pytest.raises(pkg.EkfError) as ei:
                call(bad)
            assert ei.value.status == 1 and name in str(ei.value) and "dist" in str(ei.value)
    for a, b in zip(before, (ba.nodes(), ba.points(), *ba.projections())):
        assert np.array_equal(a, b)
    with pytest.raises(pkg.EkfError):
        pkg.sba_add(np.zeros((1, 12), np.float32), [], huber=-2.0)
    # an empty handle: nothing to count, no average
    empty = pkg.BundleAdjuster(scene["camera"], capacity_nodes=2, capacity_points=2, capacity_projections=2)
    assert empty.count_bad(1.0) == 0 and empty.remove_bad(1.0) == 0 and empty.reduce_tracks() == 0
    assert empty.num_bad_points() == 0 and math.isnan(empty.avg_error()) and len(empty.projections()[0]) == 0
