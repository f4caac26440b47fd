"""The block-Jacobi PCG solver of the GPU bundle adjuster (ekf_sba_create_solver(..., EKF_SBA_SOLVER_BPCG), DESIGN.md
§11.7) against tests/sba_pcg_oracle.py, and against the Cholesky oracle where the CG is run to convergence.

A truncated CG amplifies rounding through the weak monocular gauge: with the default settings the LM trajectory of the
oracle itself differs between float64 and longdouble CG arithmetic by 4.5e-4 (poses, 11 free nodes) after 10
iterations.  So entry-wise comparisons are made with a converged CG (init_tol 1e-30, 1000 iterations) or over one
solve; a default-settings run is compared through its final cost.  Where a bound is not the 1e-9 of DESIGN.md §11.3 it
is 10 x the oracle's own float64-vs-longdouble spread, recomputed here; the figures measured on the MI355X are in
tests/golden/sba_pcg_bounds.json.
"""
import ctypes as C

import numpy as np
import pytest

import sba_oracle as so
import sba_pcg_oracle as po
import sba_robust_scene as rs
import sba_scene as sc

pytestmark = pytest.mark.gpu

NITER = 10
STATE_TOL = 1e-9          # DESIGN.md §11.3, times the scene scale
TIGHT = (1e-30, 1000)     # a CG that converges: 75-103 iterations at (11, 300), 408-712 at (59, 2000)
BIG = (1500, 30000)       # beyond the Cholesky solver's 1024 nodes; converges within 4000 CG iterations (see the test)


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def gpu_system(pkg, scene, solver="pcg", cg=None, huber=0.0):
    ba = pkg.BundleAdjuster(scene["camera"], capacity_nodes=len(scene["nodes"]), capacity_points=len(scene["points"]),
                            capacity_projections=len(scene["node"]), solver=solver)
    if cg is not None:
        ba.set_cg(*cg)
    ba.add_nodes(scene["nodes"])
    ba.add_points(scene["points"])
    ba.add_projections(scene["node"], scene["point"], scene["uv"])
    ba.huber = huber
    return ba


def state_dev(ba, ref):
    return max(float(np.abs(ba.nodes() - ref.pose7()).max()), float(np.abs(ba.points() - np.array(ref.points)).max()))


# --- 1. converged parity ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfree,npts", [(1, 40), (11, 300), (59, 2000)])
def test_converged_cg_matches_both_oracles(pkg, nfree, npts):
    """Seed 0, not test_gpu_sba.py's seed = nfree: at make_scene(11, 300, seed=11) the oracle's own float64 and
    longdouble runs of this test end 1.6e-7 apart (2.9e-11 at seed 0), so that scene cannot carry a 1e-9 bound."""
    scene = sc.make_scene(nfree, npts, seed=0)
    ref = po.pcg_system(scene).set_cg(*TIGHT)
    chol = sc.oracle_system(scene)
    ba = gpu_system(pkg, scene, cg=TIGHT)
    assert ba.solver == "pcg" and ba.get_cg() == TIGHT
    it, it_ref, it_chol = ba.run(NITER, 1e-4), ref.do_sba(NITER, 1e-4), chol.do_sba(NITER, 1e-4)
    log = ba.log()
    assert it == it_ref == it_chol
    for o in (ref, chol):
        lo = np.array(o.log, dtype=np.float64).reshape(-1, 5)
        assert np.array_equal(log[:, 3], lo[:, 3])                    # the accept / reject sequence
        assert np.array_equal(log[:, 2], lo[:, 2])
    tol = STATE_TOL * scene["scale"]
    cg_it, dn, d0 = ba.cg_log()
    print("converged parity (%d, %d): dev pcg oracle %.3g, cholesky oracle %.3g (bound %.3g); CG iterations %s"
          % (nfree, npts, state_dev(ba, ref), state_dev(ba, chol), tol, cg_it.tolist()))
    assert len(cg_it) == it and (dn < d0).all() and (cg_it < TIGHT[1]).all()
    assert state_dev(ba, ref) <= tol
    assert state_dev(ba, chol) <= tol


def test_converged_cg_matches_both_oracles_robust_after_pruning(pkg):
    scene = rs.make_robust_scene(11, 300, seed=11)
    ref = po.pcg_system(scene, 2.0).set_cg(*TIGHT)
    chol = rs.oracle_system(scene, 2.0)
    ba = gpu_system(pkg, scene, cg=TIGHT, huber=2.0)
    counts = []
    for o in (ref, chol):
        o.do_sba(NITER, 1e-4)
        counts.append((o.remove_bad(10.0), o.reduce_tracks(), o.do_sba(NITER, 1e-4)))
    ba.run(NITER, 1e-4)
    got = (ba.remove_bad(10.0), ba.reduce_tracks(), ba.run(NITER, 1e-4))
    assert got == counts[0] == counts[1] and got[0] > 0
    log = ba.log()
    for o in (ref, chol):
        assert np.array_equal(log[:, 3], np.array(o.log, dtype=np.float64).reshape(-1, 5)[:, 3])
    tol = STATE_TOL * scene["scale"]
    print("robust converged parity: dev pcg oracle %.3g, cholesky oracle %.3g (bound %.3g)"
          % (state_dev(ba, ref), state_dev(ba, chol), tol))
    assert state_dev(ba, ref) <= tol and state_dev(ba, chol) <= tol
    assert ba.count_bad(10.0) == ref.count_bad(10.0)
    assert np.isclose(ba.cost()[0], ref.calc_cost(), rtol=1e-9, atol=0)
    assert np.isclose(ba.avg_error(), ref.calc_avg_error(), rtol=1e-9, atol=0)


# --- 2. one solve with the default settings ---------------------------------------------------------------------
def test_one_default_solve_matches_the_oracle_within_its_own_rounding(pkg):
    """Measured on the MI355X (tests/golden/sba_pcg_bounds.json): see `one_default_solve` there."""
    scene = sc.make_scene(11, 300, seed=0)
    r64 = po.pcg_system(scene).set_cg(dtype=np.float64)
    r80 = po.pcg_system(scene).set_cg(dtype=np.longdouble)
    assert r64.do_sba(1, 1e-4) == r80.do_sba(1, 1e-4) == 1
    assert r64.cg_log[0][0] == r80.cg_log[0][0] == 51
    spread = max(float(np.abs(r64.pose7() - r80.pose7()).max()),
                 float(np.abs(np.array(r64.points) - np.array(r80.points)).max()))
    for o in (r64, r80):
        _, dn, d0, _ = o.cg_log[0]
        assert abs(dn - d0) > 1e-6 * d0                               # the exit test is not a coin toss
    ba = gpu_system(pkg, scene)
    assert ba.get_cg() == (1e-8, 100)
    assert ba.run(1, 1e-4) == 1
    cg_it, dn, d0 = ba.cg_log()
    dev = state_dev(ba, r64)
    print("one default solve: CG iterations %s, dn %.17g, d0 %.17g; oracle f64-vs-longdouble spread %.3g, GPU deviation "
          "%.3g (bound %.3g)" % (cg_it.tolist(), dn[0], d0[0], spread, dev, 10 * spread))
    assert cg_it.tolist() == [51]
    assert np.isclose(d0[0], r64.cg_log[0][2], rtol=1e-9, atol=0) and dn[0] < d0[0]
    assert dev <= 10 * spread


# --- 3. the residual carry-over ---------------------------------------------------------------------------------
def test_abstol_carry_over_in_the_log(pkg):
    scene = sc.make_scene(11, 300, seed=0)
    ref = po.pcg_system(scene)
    ref.do_sba(3, 1e-4)
    ba = gpu_system(pkg, scene)
    assert ba.run(3, 1e-4) == 3
    cg_it, dn, d0 = ba.cg_log()
    assert len(cg_it) == 3
    tol = ba.get_cg()[0]
    assert np.isclose(d0[0], tol * ref.cg_log[0][3], rtol=1e-9, atol=0)       # no carry-over in the first iteration
    for k in (1, 2):
        rel = tol * ref.cg_log[k][3]                 # tol dn_0 of this solve: from the oracle, the log does not hold it
        carried = dn[k - 1] / 2.0                    # from the log itself
        assert d0[k] >= carried
        if carried > 2.0 * rel:
            assert d0[k] == carried                  # bit for bit
        else:
            assert np.isclose(d0[k], max(rel, carried), rtol=1e-6, atol=0)
    assert d0[1] == dn[0] / 2.0 and d0[2] == dn[1] / 2.0     # at this scene the carried residual is the larger one
    # a new run starts without the carry-over (sba_iter = 0), the residual itself stays in the handle
    ba.run(1, 0.0)
    _, dn2, d02 = ba.cg_log()
    assert d02[0] < dn[2] / 2.0


# --- 4. a default-settings run through its final cost -------------------------------------------------------------
def test_default_run_reaches_the_oracle_cost(pkg):
    """Measured on the MI355X (tests/golden/sba_pcg_bounds.json): see `default_run_cost` there."""
    scene = sc.make_scene(59, 2000, seed=0)
    r64 = po.pcg_system(scene).set_cg(dtype=np.float64)
    r80 = po.pcg_system(scene).set_cg(dtype=np.longdouble)
    r64.do_sba(NITER, 1e-4)
    r80.do_sba(NITER, 1e-4)
    c64, c80 = r64.calc_cost(), r80.calc_cost()
    spread = abs(c64 - c80) / c64
    ba = gpu_system(pkg, scene)
    it = ba.run(NITER, 1e-4)
    cost = ba.cost()[0]
    cg_it = ba.cg_log()[0]
    dev = abs(cost - c64) / c64
    print("default run (59, 2000): oracle cost %.10g (longdouble %.10g, spread %.3g), GPU %.10g, deviation %.3g (bound "
          "%.3g); CG iterations GPU %s oracle %s" % (c64, c80, spread, cost, dev, 10 * spread, cg_it.tolist(),
                                                      [l[0] for l in r64.cg_log]))
    assert it == NITER and len(cg_it) == NITER
    assert (cg_it <= 100).all() and (cg_it == 100).any()              # the truncated path is exercised
    assert dev <= 10 * spread


# --- 5. determinism and default behaviour -------------------------------------------------------------------------
def test_two_pcg_runs_are_bitwise_identical(pkg):
    scene = sc.make_scene(59, 2000, seed=3)
    out = []
    for _ in range(2):
        ba = gpu_system(pkg, scene)
        ba.run(NITER, 1e-4)
        out.append((ba.nodes(), ba.points(), ba.log()) + ba.cg_log())
        ba.close()
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


def _raw_run(pkg, scene, create):
    lib = pkg.load_library()
    h = C.c_void_p()
    cam = pkg.sba.SbaCamera(*scene["camera"])
    assert create(lib, cam, h) == 0
    n = np.ascontiguousarray(scene["node"], np.int32)
    p = np.ascontiguousarray(scene["point"], np.int32)
    uv = np.ascontiguousarray(scene["uv"], np.float64)
    nodes, pts = np.ascontiguousarray(scene["nodes"]), np.ascontiguousarray(scene["points"])
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)                      # noqa: E731
    assert lib.ekf_sba_add_nodes(h, len(nodes), ptr(nodes)) == 0
    assert lib.ekf_sba_add_points(h, len(pts), ptr(pts)) == 0
    assert lib.ekf_sba_add_projections(h, len(n), ptr(n), ptr(p), ptr(uv), None) == 0
    it, k = C.c_int(), C.c_int()
    assert lib.ekf_sba_run(h, NITER, 1e-4, C.byref(it)) == 0
    on, op, log = np.zeros_like(nodes), np.zeros_like(pts), np.zeros((it.value, 5))
    assert lib.ekf_sba_get_nodes(h, ptr(on)) == 0 and lib.ekf_sba_get_points(h, ptr(op)) == 0
    assert lib.ekf_sba_get_log(h, it.value, ptr(log), C.byref(k)) == 0
    solver = C.c_int(-1)
    assert lib.ekf_sba_get_solver(h, C.byref(solver)) == 0 and solver.value == 0
    assert lib.ekf_sba_get_cg_log(h, 0, None, None, None, C.byref(k)) == 0 and k.value == 0
    lib.ekf_sba_destroy(h)
    return on, op, log


def test_solver_zero_is_ekf_sba_create_bit_for_bit(pkg):
    scene = sc.make_scene(59, 2000, seed=3)
    caps = (len(scene["nodes"]), len(scene["points"]), len(scene["node"]))
    a = _raw_run(pkg, scene, lambda lib, cam, h: lib.ekf_sba_create(C.byref(cam), *caps, 0, C.byref(h)))
    b = _raw_run(pkg, scene, lambda lib, cam, h: lib.ekf_sba_create_solver(C.byref(cam), *caps, 0, 0, C.byref(h)))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    # BundleAdjuster's defaults are that handle, and CG settings on it change nothing
    ba = gpu_system(pkg, scene, solver="cholesky", cg=(1e-3, 5))
    assert ba.solver == "cholesky" and ba.get_cg() == (1e-3, 5)
    ba.run(NITER, 1e-4)
    assert ba.nodes().tobytes() == a[0].tobytes() and ba.points().tobytes() == a[1].tobytes()
    assert ba.log().tobytes() == a[2].tobytes() and len(ba.cg_log()[0]) == 0
    dflt = pkg.BundleAdjuster(scene["camera"], *caps)
    assert dflt.solver == "cholesky" and dflt.get_cg() == (1e-8, 100)


def _write_files(scene, tmp_path):
    from ekf_monoslam_amd import formats
    table = np.zeros((len(scene["points"]), 12), np.float32)
    table[:, :3] = scene["points"]
    table[:, 3] = table[:, 7] = table[:, 11] = 1e-4
    recs = []
    for i, pose in enumerate(scene["nodes"]):
        sel = scene["node"] == i
        prj = np.stack([scene["point"][sel], np.floor(scene["uv"][sel, 0]), np.floor(scene["uv"][sel, 1])], 1)
        recs.append(formats.pose_record(i, pose, prj if len(prj) else None))
    (tmp_path / "points.txt").write_text(formats.format_eigen(table) + "\n")
    (tmp_path / "nodes_and_prjcts.txt").write_text("".join(recs))
    (tmp_path / "cams_cov.txt").write_text("".join(formats.camera_cov_record(np.eye(7)) for _ in recs))
    return [str(tmp_path / n) for n in ("points.txt", "nodes_and_prjcts.txt", "cams_cov.txt")]


def test_sba_add_defaults_are_the_cholesky_driver_bit_for_bit(pkg, tmp_path):
    scene = sc.make_scene(21, 300, seed=11, noise_px=0.0)
    files = _write_files(scene, tmp_path)
    a = pkg.sba_add(*files, camera=scene["camera"])
    b = pkg.sba_add(*files, camera=scene["camera"], solver="cholesky", cg_tol=1e-2, cg_max_iters=3)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    # and the PCG driver, converged, lands where the Cholesky oracle driver does
    from ekf_monoslam_amd import formats
    c = pkg.sba_add(*files, camera=scene["camera"], solver="pcg", cg_tol=TIGHT[0], cg_max_iters=TIGHT[1])
    ref, rows, _ = so.sba_add(formats.read_points(files[0]), formats.read_pose_records(files[1]), camera=scene["camera"])
    tol = 1e-6 * scene["scale"]                                       # test_gpu_sba.py's bound for the driver
    np.testing.assert_allclose(c[0][rows], np.array(ref.points), rtol=0, atol=tol)
    np.testing.assert_allclose(c[1], ref.pose7(), rtol=0, atol=tol)


# --- 6. beyond the 1024-node limit of the Cholesky solver ---------------------------------------------------------
def test_pcg_runs_beyond_the_cholesky_cap(pkg):
    """make_scene(1500, 30000), init_tol 1e-30, at most 4000 CG iterations, 3 LM iterations.  On the CPU the oracle's
    solves at this size converge in well under 4000 iterations (asserted below), so the size of the issue is used."""
    scene = sc.make_scene(*BIG, seed=0)
    cg = (1e-30, 4000)
    ref = po.pcg_system(scene).set_cg(*cg)
    it_ref = ref.do_sba(3, 1e-4)
    assert all(l[0] < cg[1] and l[1] < l[2] for l in ref.cg_log), ref.cg_log
    with pytest.raises(pkg.EkfError) as ei:
        gpu_system(pkg, scene, solver="cholesky")
    assert ei.value.status == 1 and "1024" in str(ei.value)
    ba = gpu_system(pkg, scene, cg=cg)
    it = ba.run(3, 1e-4)
    log = ba.log()
    cg_it, dn, d0 = ba.cg_log()
    dev = state_dev(ba, ref)
    print("beyond the cap %s: CG iterations GPU %s oracle %s; deviation from the oracle %.3g (bound %.3g)"
          % (BIG, cg_it.tolist(), [l[0] for l in ref.cg_log], dev, STATE_TOL * scene["scale"]))
    assert it == it_ref == 3 and (dn < d0).all() and (cg_it < cg[1]).all()
    acc = log[:, 3] == 1
    assert acc.any() and (log[acc, 1] < log[acc, 0]).all()
    assert np.array_equal(log[:, 3], np.array(ref.log, dtype=np.float64).reshape(-1, 5)[:, 3])
    assert dev <= STATE_TOL * scene["scale"]


def test_sba_add_driver_with_more_than_1024_records(pkg, tmp_path):
    scene = sc.make_scene(1100, 11000, seed=2, noise_px=0.0)
    files = _write_files(scene, tmp_path)
    with pytest.raises(pkg.EkfError) as ei:
        pkg.sba_add(*files, camera=scene["camera"], every=0)
    assert ei.value.status == 1
    out, nodes, ids = pkg.sba_add(*files, camera=scene["camera"], every=200, solver="pcg")
    assert ids == list(range(1101)) and nodes.shape == (1101, 7) and np.isfinite(nodes).all() and np.isfinite(out).all()

    # The monocular gauge is free (only node 0 is fixed), so the result is judged by its reprojection error, not by
    # the distance to the true poses: the keypoints were floored to whole pixels, the start is 0.01 / 0.02 off.
    def rms(nd, pts):
        ba = pkg.BundleAdjuster(scene["camera"], capacity_nodes=1101, capacity_points=len(pts),
                                capacity_projections=len(scene["node"]), solver="pcg")
        ba.add_nodes(nd)
        ba.add_points(pts)
        ba.add_projections(scene["node"], scene["point"], np.floor(scene["uv"]))
        return ba.rms_cost()

    rms0 = rms(scene["nodes"].astype(np.float32), scene["points"].astype(np.float32))
    rms1 = rms(nodes, out)
    print("sba_add, 1101 records, pcg: rms reprojection error %.3g -> %.3g px" % (rms0, rms1))
    # LM only accepts steps that lower the cost, so the error can only fall; with the default 100 CG iterations the
    # solves of a 1100-node chain are far from converged and it falls slowly (measured on the MI355X: 11.1 -> 10.4 px).
    assert rms1 < rms0


# --- 7. errors ------------------------------------------------------------------------------------------------------
def test_non_positive_block_pivot_is_reported_and_keeps_the_state(pkg):
    # test_gpu_sba.py's case: node 1 at the origin sees a point at the origin, its Jacobians are NaN
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
    assert ei.value.status == 5 and "diagonal block" in str(ei.value)      # EKF_ERR_NUMERIC
    assert np.array_equal(ba.nodes(), n0) and np.array_equal(ba.points(), p0)
    with pytest.raises(so.NotPositiveDefinite):
        po.pcg_system(scene).do_sba(NITER, 1e-4)


def test_bad_arguments(pkg):
    scene = sc.make_scene(3, 40, seed=5)
    ba = gpu_system(pkg, scene)
    for tol, mx in ((-1.0, 10), (np.nan, 10), (np.inf, 10), (1e-8, 0), (1e-8, -3)):
        with pytest.raises(pkg.EkfError) as ei:
            ba.set_cg(tol, mx)
        assert ei.value.status == 1 and "set_cg" in str(ei.value)
    assert ba.get_cg() == (1e-8, 100)
    with pytest.raises(ValueError):
        pkg.BundleAdjuster(scene["camera"], solver="gradient")
    lib = pkg.load_library()
    h = C.c_void_p()
    cam = pkg.sba.SbaCamera(*scene["camera"])
    for solver in (1, 2, 4, -1):
        assert lib.ekf_sba_create_solver(C.byref(cam), 10, 10, 10, 0, solver, C.byref(h)) == 1
        assert b"solver" in lib.ekf_sba_last_error(None) and not h
    # a PCG handle takes a capacity the Cholesky solver refuses, and nothing is allocated for it up front
    big = pkg.BundleAdjuster(scene["camera"], capacity_nodes=100000, capacity_points=10, capacity_projections=10,
                             solver="pcg")
    assert big.solver == "pcg" and big.run(1, 1e-4) == -1 and len(big.cg_log()[0]) == 0
