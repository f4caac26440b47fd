"""GPU bundle adjustment (ekf_sba_*) on camera systems that are not a narrow band: the scenes of
tests/sba_topology_scene.py (dense, loop closure, hub node, two islands) against the numpy oracles.

tests/test_gpu_sba.py, test_gpu_sba_robust.py and test_gpu_sba_pcg.py only ever build block-banded systems of a
half-bandwidth of at most 5 blocks, narrower than one 64-wide Cholesky tile.  Here the trailing update and the panel of
sba_chol_f64 work on non-zero tiles far from the diagonal, k_sba_trsv sweeps full columns, the pair kernels mirror
blocks between far tiles, the zeroing of the dense matrix matters (absent blocks, blocks that disappear after
pruning), k_sba_cg_mv walks long neighbour lists across workgroups, and one thread of k_sba_point walks up to 60
projections.

Bounds (tests/golden/sba_topology_bounds.json holds the oracle spreads, the seeds and the deviations measured on the
MI355X).  COST_RTOL and STATE_TOL are tests/test_gpu_sba.py's, PCG_TOL is DESIGN.md §11.3's 1e-9 of
tests/test_gpu_sba_pcg.py.  A scene carries them only if 10 x the oracle's own rounding spread (float64 solve against
longdouble solve, asserted on the CPU by tests/test_oracle_sba_topology.py) is below them; the scenes listed in
`sba_topology_scene.OWN_BOUND` do not, and their bound is 10 x that spread, recomputed here.  The accept / reject
column can be exact because no oracle decision is a near-tie (also asserted on the CPU).
"""
import ctypes as C

import numpy as np
import pytest

import sba_topology_scene as ts

pytestmark = pytest.mark.gpu

NITER = ts.NITER          # 5: later iterations of a dense scene change the cost by less than 1e-6 of it (coin tosses)
COST_RTOL = 1e-9          # per-iteration costs (tests/test_gpu_sba.py)
STATE_TOL = 1e-8          # final nodes and points, times the scene scale (tests/test_gpu_sba.py)
PCG_TOL = 1e-9            # converged CG against both oracles, times the scene scale
TIGHT = ts.PCG_TIGHT      # init_tol 1e-30 as tests/test_gpu_sba_pcg.py; 4000 iterations: loop at F = 127 needs 2497
HUBER = 2.0
DIST = 10.0
MARGIN = 1e-6             # tests/test_gpu_sba_robust.py: no oracle e^2 this close (relative) to DIST^2


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def gpu_system(pkg, scene, solver="cholesky", cg=None, huber=0.0, keep=None, capacity_nodes=None):
    ba = pkg.BundleAdjuster(scene["camera"], capacity_nodes=capacity_nodes or len(scene["nodes"]),
                            capacity_points=len(scene["points"]), capacity_projections=len(scene["node"]), solver=solver)
    if cg is not None:
        ba.set_cg(*cg)
    ba.add_nodes(scene["nodes"])
    ba.add_points(scene["points"])
    sel = slice(None) if keep is None else keep
    ba.add_projections(scene["node"][sel], scene["point"][sel], scene["uv"][sel])
    ba.huber = huber
    return ba


def state_dev(ba, ref):
    return max(float(np.abs(ba.nodes() - ref.pose7()).max()), float(np.abs(ba.points() - np.array(ref.points)).max()))


def assert_log_matches(ba, it, ref, it_ref, costs=True):
    log, log_ref = ba.log(), np.array(ref.log, dtype=np.float64).reshape(-1, 5)
    assert it == it_ref and log.shape == log_ref.shape
    assert np.array_equal(log[:, 3], log_ref[:, 3])                  # accept / reject sequence
    assert np.array_equal(log[:, 2], log_ref[:, 2])                  # lambda: exact halvings / doublings
    if costs:
        np.testing.assert_allclose(log[:, :2], log_ref[:, :2], rtol=COST_RTOL, atol=0)


def state_bound(case, scene, project_tol, spread_of):
    """The project bound, or for a scene of OWN_BOUND 10 x the oracle's float64-vs-longdouble spread (`spread_of()`)."""
    tol = project_tol * scene["scale"]
    if tuple(case) in ts.OWN_BOUND:
        spread = spread_of()
        print("own bound for %s: oracle spread %.3g, bound %.3g (project bound %.3g)" % (case, spread, 10 * spread, tol))
        tol = max(tol, 10 * spread)
    return tol


def chol_spread(scene, niter=NITER, huber=None):
    a, b = ts.cholesky_oracle(scene, huber), ts.cholesky_oracle(scene, huber, longdouble=True)
    a.do_sba(niter, 1e-4)
    b.do_sba(niter, 1e-4)
    return ts.state_spread(a, b)


# --- 1. the Cholesky handle on every kind ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nfree,npts,seed", ts.CHOL_CASES)
def test_cholesky_run_matches_oracle(pkg, kind, nfree, npts, seed):
    """npad = ceil(6 F / 64) 64: F = 10 is one tile (no panel, no trailing launch), 11 the first panel, 32 is 192 with
    no padding rows, 59 and 127 are 384 and 768.  Measured: `cholesky` in tests/golden/sba_topology_bounds.json."""
    case = (kind, nfree, npts, seed)
    scene = ts.case_scene(*case)
    ref = ts.cholesky_oracle(scene)
    ba = gpu_system(pkg, scene)
    assert ba.counts() == (len(ref.trans), len(ref.points), ref.nprojs)
    c0, r0 = ba.cost()
    assert np.isclose(c0, ref.calc_cost(), rtol=COST_RTOL, atol=0)
    assert np.isclose(r0, ref.calc_rms_cost(), rtol=COST_RTOL, atol=0)
    it, it_ref = ba.run(NITER, 1e-4), ref.do_sba(NITER, 1e-4)
    tol = state_bound(case, scene, STATE_TOL, lambda: chol_spread(scene))
    log, log_ref = ba.log(), np.array(ref.log, dtype=np.float64).reshape(-1, 5)
    print("cholesky %s: deviation %.3g (bound %.3g), max cost rel. deviation %.3g"
          % (case, state_dev(ba, ref), tol, float(np.abs(log[:, :2] / log_ref[:, :2] - 1).max())
             if log.shape == log_ref.shape else np.nan))
    assert_log_matches(ba, it, ref, it_ref)
    assert state_dev(ba, ref) <= tol
    assert ba.rms_cost() < r0
    ba.close()


def test_cholesky_handle_at_its_cap(pkg):
    """1024 nodes: n6 = 6138, npad = 6144 = kSbaMaxN, every element of k_sba_trsv's LDS vector in use; a loop scene
    with short tracks, two LM iterations.  Measured: `cap` in tests/golden/sba_topology_bounds.json."""
    kind, nfree, npts, seed = ts.CAP_CASE
    scene = ts.case_scene(kind, nfree, npts, seed)
    assert len(scene["nodes"]) == 1024
    # one node more: the handle refuses it (EKF_ERR_CAPACITY), and no Cholesky handle can be made for it (EKF_ERR_ARG)
    ba = gpu_system(pkg, scene)
    with pytest.raises(pkg.EkfError) as ei:
        ba.add_nodes(scene["nodes"][:1])
    assert ei.value.status == 2 and ba.counts()[0] == 1024            # EKF_ERR_CAPACITY
    with pytest.raises(pkg.EkfError) as ei:
        pkg.BundleAdjuster(scene["camera"], capacity_nodes=1025, capacity_points=10, capacity_projections=10)
    assert ei.value.status == 1 and "1024" in str(ei.value)
    ref = ts.cholesky_oracle(scene)
    c0 = ba.cost()[0]
    assert np.isclose(c0, ref.calc_cost(), rtol=COST_RTOL, atol=0)
    it, it_ref = ba.run(2, 1e-4), ref.do_sba(2, 1e-4)
    tol = state_bound(ts.CAP_CASE, scene, STATE_TOL, lambda: chol_spread(scene, 2))
    print("cholesky at the cap %s: deviation %.3g (bound %.3g)" % (ts.CAP_CASE, state_dev(ba, ref), tol))
    assert it == 2
    assert_log_matches(ba, it, ref, it_ref)
    assert state_dev(ba, ref) <= tol
    ba.close()


# --- 2. the PCG handle ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nfree,npts,seed", ts.PCG_CASES)
def test_converged_cg_matches_both_oracles(pkg, kind, nfree, npts, seed):
    """F = 41, 42, 43: one kSbaCgRows group of block rows, exactly and just over; 127: four groups, neighbours up to
    three groups away.  Measured: `pcg` in tests/golden/sba_topology_bounds.json."""
    case = (kind, nfree, npts, seed)
    scene = ts.case_scene(*case)
    ref, chol = ts.pcg_oracle(scene, TIGHT), ts.cholesky_oracle(scene)
    ba = gpu_system(pkg, scene, solver="pcg", cg=TIGHT)
    it, it_ref, it_chol = ba.run(NITER, 1e-4), ref.do_sba(NITER, 1e-4), chol.do_sba(NITER, 1e-4)

    def spread():
        r80 = ts.pcg_oracle(scene, TIGHT, longdouble=True)
        r80.do_sba(NITER, 1e-4)
        return max(ts.state_spread(ref, r80), chol_spread(scene))

    tol = state_bound(case, scene, PCG_TOL, spread)
    cg_it, dn, d0 = ba.cg_log()
    print("pcg %s: deviation from the pcg oracle %.3g, from the cholesky oracle %.3g (bound %.3g); CG iterations %s"
          % (case, state_dev(ba, ref), state_dev(ba, chol), tol, cg_it.tolist()))
    assert it_ref == it_chol
    for o in (ref, chol):
        assert_log_matches(ba, it, o, it_ref, costs=False)
    assert len(cg_it) == it and (dn < d0).all() and (cg_it < TIGHT[1]).all()
    assert state_dev(ba, ref) <= tol
    assert state_dev(ba, chol) <= tol
    ba.close()


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
    lib.ekf_sba_destroy(h)
    return on, op, log


def test_solver_zero_is_ekf_sba_create_bit_for_bit_on_a_dense_scene(pkg):
    scene = ts.case_scene(*ts.BITWISE_CASE)
    caps = (len(scene["nodes"]), len(scene["points"]), len(scene["node"]))
    a = _raw_run(pkg, scene, lambda lib, cam, h: lib.ekf_sba_create(C.byref(cam), *caps, 0, C.byref(h)))
    b = _raw_run(pkg, scene, lambda lib, cam, h: lib.ekf_sba_create_solver(C.byref(cam), *caps, 0, 0, C.byref(h)))
    assert len(a[2]) > 0
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("solver", ["cholesky", "pcg"])
def test_two_runs_on_a_dense_scene_are_bitwise_identical(pkg, solver):
    scene = ts.case_scene(*ts.BITWISE_CASE)
    out = []
    for _ in range(2):
        ba = gpu_system(pkg, scene, solver=solver)
        ba.run(NITER, 1e-4)
        out.append((ba.nodes(), ba.points(), ba.log()) + ba.cg_log())
        ba.close()
    assert len(out[0][2]) > 0
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


# --- 3. the robust path on a dense scene ----------------------------------------------------------------------------
def _robust_scene():
    return ts.make_topology_scene(**ts.ROBUST_CASE)


def test_huber_and_pruning_on_a_dense_scene_match_the_oracle(pkg):
    """huber = 2, run, remove_bad(10), reduce_tracks, run again (the sequence of
    test_converged_cg_matches_both_oracles_robust_after_pruning) on the Cholesky handle against RobustSysSBA, with
    exact counts.  The outliers of the doomed pairs remove every point those far pairs share: their blocks are in the
    first system and must be zero in the second.  Measured: `robust` in tests/golden/sba_topology_bounds.json."""
    scene = _robust_scene()
    ref = ts.cholesky_oracle(scene, HUBER)
    ba = gpu_system(pkg, scene, huber=HUBER)
    before = ts.pair_set(*ba.projections()[:2])
    assert all((a - 1, b - 1) in before for a, b in scene["doomed"])
    it, it_ref = ba.run(NITER, 1e-4), ref.do_sba(NITER, 1e-4)
    assert_log_matches(ba, it, ref, it_ref)
    assert float(np.min(np.abs(ref.errors() / (DIST * DIST) - 1.0))) > MARGIN   # no count can flip on rounding
    got = (ba.remove_bad(DIST), ba.reduce_tracks())
    assert got == (ref.remove_bad(DIST), ref.reduce_tracks()) and got[0] > 0
    for x, y in zip(ba.projections(), ref.projections()):
        assert np.array_equal(x, y)
    after = ts.pair_set(*ba.projections()[:2])
    gone = before - after
    doomed_gone = sum((a - 1, b - 1) in gone for a, b in scene["doomed"])
    assert after < before and max(b - a for a, b in gone) > 42        # far blocks disappear between the two runs
    it, it_ref = ba.run(NITER, 1e-4), ref.do_sba(NITER, 1e-4)
    assert_log_matches(ba, it, ref, it_ref)
    tol = STATE_TOL * scene["scale"]
    print("robust dense: %d pairs before, %d gone after pruning (%d of the %d doomed ones); deviation %.3g (bound %.3g)"
          % (len(before), len(gone), doomed_gone, len(scene["doomed"]), state_dev(ba, ref), tol))
    assert state_dev(ba, ref) <= tol
    assert ba.count_bad(DIST) == ref.count_bad(DIST)
    assert np.isclose(ba.cost()[0], ref.calc_cost(), rtol=COST_RTOL, atol=0)
    ba.close()


def test_pruned_equals_rebuilt_bit_for_bit_on_a_dense_scene(pkg):
    """test_gpu_sba_robust.py's comparison where pruning removes whole pair blocks: a handle that assembled the larger
    system first and one that never held those pairs give the same bits."""
    scene = _robust_scene()
    a = gpu_system(pkg, scene, huber=HUBER)
    before = ts.pair_set(*a.projections()[:2])
    removed = a.remove_bad(DIST)
    assert removed > 0
    a.reduce_tracks()
    node, point, uv, valid = a.projections()
    assert valid.all() and len(node) < len(scene["node"])
    assert len(before - ts.pair_set(node, point)) > 0                 # pair blocks disappear
    stored = set(zip(node.tolist(), point.tolist()))
    keep = np.array([(int(n), int(p)) in stored for n, p in zip(scene["node"], scene["point"])])
    first = {}
    for k, key in enumerate(zip(scene["node"].tolist(), scene["point"].tolist())):
        keep[k] = keep[k] and first.setdefault(key, k) == k           # a repeat keeps the first keypoint
    assert keep.sum() == len(node)
    b = gpu_system(pkg, scene, huber=HUBER, keep=keep)
    for x, y in zip(a.projections(), b.projections()):
        assert np.array_equal(x, y)
    ca, cb = a.cost(), b.cost()
    ia, ib = a.run(NITER, 1e-4), b.run(NITER, 1e-4)
    assert ia == ib and ia > 0 and ca == cb
    for x, y in ((a.nodes(), b.nodes()), (a.points(), b.points()), (a.log(), b.log())):
        assert x.tobytes() == y.tobytes()
    a.close()
    b.close()


# --- 4. one LM iteration: the solve's x and the point back-substitution, without LM's self-correction --------------
@pytest.mark.parametrize("solver", ["cholesky", "pcg"])
@pytest.mark.parametrize("kind,nfree,npts,seed", ts.ONE_STEP_CASES)
def test_one_iteration_matches_oracle(pkg, solver, kind, nfree, npts, seed):
    """Measured: `one_step` in tests/golden/sba_topology_bounds.json."""
    scene = ts.case_scene(kind, nfree, npts, seed)
    pcg = solver == "pcg"
    ref = ts.pcg_oracle(scene, TIGHT) if pcg else ts.cholesky_oracle(scene)
    ba = gpu_system(pkg, scene, solver=solver, cg=TIGHT if pcg else None)
    it, it_ref = ba.run(1, 1e-4), ref.do_sba(1, 1e-4)
    assert it == 1
    assert_log_matches(ba, it, ref, it_ref, costs=not pcg)
    log, log_ref = ba.log(), np.array(ref.log, dtype=np.float64).reshape(-1, 5)
    tol = (PCG_TOL if pcg else STATE_TOL) * scene["scale"]
    print("one iteration %s %s: deviation %.3g (bound %.3g), |x|^2 %.17g against %.17g"
          % (solver, (kind, nfree, npts, seed), state_dev(ba, ref), tol, log[0, 4], log_ref[0, 4]))
    assert state_dev(ba, ref) <= tol
    ba.close()


@pytest.mark.parametrize("solver", ["cholesky", "pcg"])
def test_a_quiet_island_stays_where_it_is(pkg, solver):
    """islands with the second island at the truth and noise-free: its right-hand side is rounding, no block couples it
    to the first island, so one LM iteration moves the first island's nodes and leaves the second island's within
    the bound.  Anything that leaks between the islands (a tile of the trailing update written to the wrong place, an
    absent block that is not zero, a neighbour list that crosses over) moves them."""
    kind, nfree, npts, seed = ts.ONE_STEP_CASES[1]
    assert kind == "islands"
    scene = ts.case_scene(kind, nfree, npts, seed, quiet_second=True)
    first, second = ts.island_groups(nfree)
    pcg = solver == "pcg"
    ba = gpu_system(pkg, scene, solver=solver, cg=TIGHT if pcg else None)
    n0 = ba.nodes()
    assert ba.run(1, 1e-4) == 1 and ba.log()[0, 3] == 1
    moved = np.abs(ba.nodes() - n0).max(axis=1)
    tol = (PCG_TOL if pcg else STATE_TOL) * scene["scale"]
    print("quiet island, %s: first island moves %.3g .. %.3g, second at most %.3g (bound %.3g)"
          % (solver, moved[first].min(), moved[first].max(), moved[second].max(), tol))
    assert moved[second].max() <= tol
    assert moved[first].min() > 1e3 * tol
    ba.close()
