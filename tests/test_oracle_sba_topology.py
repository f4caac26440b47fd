"""CPU checks of tests/sba_topology_scene.py and of the oracle-side conditions tests/test_gpu_sba_topology.py relies on.

1. Structure: every scene the GPU tests use has the matrix structure it is there for (computed from scene["node"] and
   scene["point"] alone), so that a change of the generator back towards consecutive tracks fails here.
2. The oracles run on these scenes and lower the RMS cost.
3. Bounds: a GPU test may assert a project bound (STATE_TOL = 1e-8 x scale for a Cholesky handle, 1e-9 x scale for a
   converged CG) on a scene only if 10 x the oracle's own rounding spread -- its final state with the float64 solve
   against the same run with the solve in longdouble (sba_oracle.solve_refined, sba_pcg_oracle's dtype) -- is below it;
   the factor 10 is the margin of helpers.bound and tests/golden/sba_pcg_bounds.json for a device that sums in another
   order.  Scenes in sba_topology_scene.OWN_BOUND are exempt (their GPU bound is 10 x the spread itself).
4. Ties: every accept / reject decision of every oracle run has |newcost - cost| > 1e-6 cost, so the GPU's accept /
   reject column can be compared exactly.  That is why the runs have 5 iterations: from about the seventh on a dense
   scene has converged and changes its cost by 1e-7 .. 1e-9 of it (measured: tests/golden/sba_topology_bounds.json).
"""
import functools

import numpy as np
import pytest

import sba_oracle as so
import sba_topology_scene as ts

STATE_TOL = 1e-8          # tests/test_gpu_sba.py
PCG_TOL = 1e-9
TIE = 1e-6
ALL_CASES = sorted(set(ts.CHOL_CASES) | set(ts.PCG_CASES) | set(ts.ONE_STEP_CASES) | {ts.BITWISE_CASE})


@functools.lru_cache(maxsize=None)
def chol_runs(case, niter=ts.NITER):
    """(float64 oracle, longdouble-solve oracle, start RMS) after do_sba(niter, 1e-4)."""
    scene = ts.case_scene(*case)
    a, b = ts.cholesky_oracle(scene), ts.cholesky_oracle(scene, longdouble=True)
    r0 = a.calc_rms_cost()
    assert a.do_sba(niter, 1e-4) == b.do_sba(niter, 1e-4) == niter
    return a, b, r0, scene["scale"]


def assert_no_tie_and_same_decisions(*oracles):
    logs = [np.array(o.log, dtype=np.float64).reshape(-1, 5) for o in oracles]
    for o, log in zip(oracles, logs):
        assert ts.tie_margin(o) > TIE, log[:, :2]
        assert np.array_equal(log[:, 2:4], logs[0][:, 2:4])           # lambda and accept / reject


# --- 1. structure ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,nfree,npts,seed", ALL_CASES + [ts.CAP_CASE])
def test_structure(kind, nfree, npts, seed):
    scene = ts.case_scene(kind, nfree, npts, seed)
    st = ts.structure(scene)
    nseen = len(st["seen_free"])
    assert nseen == nfree - 1 and nfree - 1 not in st["seen_free"]    # the last free node has no projection
    assert len(scene["node"]) - len(set(zip(scene["node"].tolist(), scene["point"].tolist()))) == 5   # the repeats
    assert len(scene["nodes"]) == nfree + 1 and len(scene["points"]) == npts
    if kind == "dense":
        assert st["pair_fraction"] == 1.0 and st["max_span"] == nseen - 1 and st["max_degree"] == nseen - 1
        assert st["longest_track"] >= min(nseen, 50)
    elif kind == "loop":
        assert st["max_span"] >= nseen - 4 and st["pair_fraction"] < 0.6 and st["longest_track"] <= 4
        far = [p for p in st["pairs"] if p[1] - p[0] >= nseen - 8]
        assert len(far) >= 4                                          # the corner block
        assert all(b - a <= 3 or b - a >= nseen - 8 for a, b in st["pairs"])   # A itself: a band and the corner
    elif kind == "hub":
        assert st["max_degree"] >= 0.9 * (nseen - 1) and st["longest_track"] <= 4
        hub = int(np.argmax(st["degree"]))
        assert all(b - a <= 2 or hub in (a, b) for a, b in st["pairs"])        # an arrow
        assert sorted(st["degree"])[-2] <= 5
    else:
        first, second = ts.island_groups(nfree)
        f, s = {i - 1 for i in first}, {i - 1 for i in second}
        assert f | s == set(st["seen_free"]) and not f & s and min(len(f), len(s)) >= nseen // 2
        assert not any((a in f) != (b in f) for a, b in st["pairs"])  # the absent block
        inside = len(f) * (len(f) - 1) // 2 + len(s) * (len(s) - 1) // 2
        assert st["n_pairs"] >= 0.8 * inside and st["max_span"] >= len(f) - 3 and st["longest_track"] >= 8


def test_dense_pairs_have_long_item_lists_and_far_tiles():
    scene = ts.case_scene(*ts.BITWISE_CASE)
    node, point = scene["node"], scene["point"]
    shared = len(set(point[node == 1].tolist()) & set(point[node == 120].tolist()))
    assert shared >= 5                                                # items of the pair block (0, 119): tiles 0 and 11
    st = ts.structure(scene)
    assert st["max_span"] > 2 * 42                                    # neighbours two kSbaCgRows groups away


def test_kind_is_checked():
    with pytest.raises(ValueError):
        ts.make_topology_scene("band", 5, 40)


# --- 2.-4. the oracle runs, its rounding spread, its decisions -------------------------------------------------------
@pytest.mark.parametrize("kind,nfree,npts,seed", ts.CHOL_CASES)
def test_cholesky_oracle_spread_and_ties(kind, nfree, npts, seed):
    case = (kind, nfree, npts, seed)
    a, b, r0, scale = chol_runs(case)
    spread = ts.state_spread(a, b)
    print("cholesky %s: rms %.3g -> %.3g, spread %.3g, tie margin %.3g" % (case, r0, a.calc_rms_cost(), spread,
                                                                           ts.tie_margin(a)))
    assert a.calc_rms_cost() < 0.1 * r0
    assert_no_tie_and_same_decisions(a, b)
    if case not in ts.OWN_BOUND:
        assert 10 * spread <= STATE_TOL * scale


@pytest.mark.parametrize("kind,nfree,npts,seed", ts.PCG_CASES)
def test_pcg_oracle_spread_and_ties(kind, nfree, npts, seed):
    case = (kind, nfree, npts, seed)
    scene = ts.case_scene(*case)
    p64, p80 = ts.pcg_oracle(scene, ts.PCG_TIGHT), ts.pcg_oracle(scene, ts.PCG_TIGHT, longdouble=True)
    assert p64.do_sba(ts.NITER, 1e-4) == p80.do_sba(ts.NITER, 1e-4) == ts.NITER
    c64, c80, r0, scale = chol_runs(case)
    spread = max(ts.state_spread(p64, p80), ts.state_spread(c64, c80))
    print("pcg %s: spread pcg %.3g, cholesky %.3g, pcg against cholesky %.3g; CG iterations %s"
          % (case, ts.state_spread(p64, p80), ts.state_spread(c64, c80), ts.state_spread(p64, c64),
             [l[0] for l in p64.cg_log]))
    assert all(l[0] < ts.PCG_TIGHT[1] and l[1] < l[2] for l in p64.cg_log + p80.cg_log)       # the CG converged
    assert p64.calc_rms_cost() < 0.1 * r0
    assert_no_tie_and_same_decisions(p64, p80, c64, c80)
    if case not in ts.OWN_BOUND:
        assert 10 * spread <= PCG_TOL * scale


def test_cap_oracle_spread_and_ties():
    a, b, r0, scale = chol_runs(ts.CAP_CASE, 2)
    spread = ts.state_spread(a, b)
    print("cap %s: rms %.3g -> %.3g, spread %.3g" % (ts.CAP_CASE, r0, a.calc_rms_cost(), spread))
    assert a.calc_rms_cost() < r0
    assert_no_tie_and_same_decisions(a, b)
    assert 10 * spread <= STATE_TOL * scale


@pytest.mark.parametrize("kind,nfree,npts,seed", ts.ONE_STEP_CASES)
def test_one_iteration_oracle_spread(kind, nfree, npts, seed):
    case = (kind, nfree, npts, seed)
    a, b, r0, scale = chol_runs(case, 1)
    scene = ts.case_scene(*case)
    p64, p80 = ts.pcg_oracle(scene, ts.PCG_TIGHT), ts.pcg_oracle(scene, ts.PCG_TIGHT, longdouble=True)
    assert p64.do_sba(1, 1e-4) == p80.do_sba(1, 1e-4) == 1
    assert_no_tie_and_same_decisions(a, b, p64, p80)
    assert 10 * ts.state_spread(a, b) <= STATE_TOL * scale
    assert 10 * max(ts.state_spread(p64, p80), ts.state_spread(a, b)) <= PCG_TOL * scale


def test_robust_scene_loses_far_pairs_and_keeps_its_bound():
    scene = ts.make_topology_scene(**ts.ROBUST_CASE)
    st = ts.structure(scene)
    assert st["pair_fraction"] > 0.9 and scene["outlier"].sum() > 0.03 * len(scene["node"])
    before = st["pairs"]
    assert len(scene["doomed"]) == 6 and all((a - 1, b - 1) in before and b - a > 39 for a, b in scene["doomed"])
    runs = []
    for ld in (False, True):
        s = ts.cholesky_oracle(scene, 2.0, longdouble=ld)
        assert s.do_sba(ts.NITER, 1e-4) == ts.NITER
        first = np.array(s.log, dtype=np.float64).reshape(-1, 5)
        assert ts.tie_margin(s) > TIE
        assert float(np.min(np.abs(s.errors() / 100.0 - 1.0))) > 1e-6           # remove_bad(10) cannot flip on rounding
        counts = (s.remove_bad(10.0), s.reduce_tracks())
        node, point, _, valid = s.projections()
        gone = before - ts.pair_set(node, point)
        assert valid.all() and counts[0] > 0 and len(gone) > 0 and max(b - a for a, b in gone) > 42
        assert s.do_sba(ts.NITER, 1e-4) == ts.NITER
        assert ts.tie_margin(s) > TIE
        runs.append((s, counts, first[:, 2:4].tolist(), np.array(s.log)[:, 2:4].tolist()))
    assert runs[0][1:] == runs[1][1:]
    assert 10 * ts.state_spread(runs[0][0], runs[1][0]) <= STATE_TOL * scene["scale"]
    # pruning at the start state (the bit-for-bit comparison of the GPU test) removes whole pair blocks as well
    s = ts.cholesky_oracle(scene, 2.0)
    assert s.remove_bad(10.0) > 0
    s.reduce_tracks()
    node, point, _, _ = s.projections()
    assert len(before - ts.pair_set(node, point)) > 0


def test_quiet_island_does_not_move_in_the_oracle():
    kind, nfree, npts, seed = ts.ONE_STEP_CASES[1]
    scene = ts.case_scene(kind, nfree, npts, seed, quiet_second=True)
    first, second = ts.island_groups(nfree)
    for o in (ts.cholesky_oracle(scene), ts.pcg_oracle(scene, ts.PCG_TIGHT)):
        n0 = o.pose7().copy()
        assert o.do_sba(1, 1e-4) == 1 and o.log[0][3] == 1
        moved = np.abs(o.pose7() - n0).max(axis=1)
        assert moved[second].max() <= 0.1 * PCG_TOL * scene["scale"]          # rounding: 1e-15 measured
        assert moved[first].min() > 1e3 * STATE_TOL * scene["scale"]


def test_refined_solve_is_the_longdouble_solve():
    rng = np.random.default_rng(0)
    M = rng.normal(size=(40, 40))
    A = M @ M.T + 1e-3 * np.eye(40)                                  # cond ~ 1e5
    x_true = rng.normal(size=40)
    B = (A.astype(np.longdouble) @ x_true.astype(np.longdouble)).astype(np.float64)
    e_ref = np.abs(so.solve_refined(A, B) - x_true).max()
    e_f64 = np.abs(so.SysSBA.solve(A, B) - x_true).max()
    assert e_ref <= e_f64 + 1e-13 and e_ref < 1e-9
    with pytest.raises(so.NotPositiveDefinite):
        so.solve_refined(-np.eye(3), np.ones(3))
