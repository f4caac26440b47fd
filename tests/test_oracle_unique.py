"""The runner-up cost and the uniqueness test in tests/unique_oracle.py alone: the definition against a
one-pass restatement, the small plane counts, the filter's two ends, the defect of the geometric filter on the flat-patch
scenes and its cure, the aggregated sweeps, and the prototype table.  CPU only."""
import inspect

import numpy as np
import pytest

import dense_oracle as do
import dense_scene as ds
import sgm_scene as ss
import unique_oracle as uo
import unique_scene as us

ARGS = (ds.W_MIN, ds.W_MAX)


def _curve(case):
    name, w, h, D, radius, trunc, src, census, n_best, paths, p1, p2, _ = case
    v = us.case_views(case)
    return uo.volume(v[0][0], v[0][1], v[0][2], [v[s] for s in src], *ARGS, D, radius, trunc, bool(census), n_best, paths, p1, p2)


@pytest.mark.parametrize("case", us.CASES, ids=[c[0] for c in us.CASES])
def test_brute_force_equals_the_one_pass_top_four(case):
    C, V = _curve(case)
    want = uo.runner_up(C)
    got, ks, c1 = uo.runner_up_top4(C)
    w = do.winner(C, V, *ARGS)
    print(case[0], "absent:", int((want == uo.ABSENT).sum()), "of", want.size, "flat:", int((want == w["cost"]).sum()))
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert np.array_equal(ks, np.argmin(C, axis=0)) and np.array_equal(c1.astype(np.uint32), w["cost"])    # the free cross-check
    assert (want.astype(np.int64) >= w["cost"].astype(np.int64)).all()
    # ... and pixel by pixel, plane by plane, on a few pixels
    D, H, W = C.shape
    for y, x in ((0, 0), (H - 1, W - 1), (H // 2, W // 3)):
        k0 = min(range(D), key=lambda k: (int(C[k, y, x]), k))
        far = [int(C[k, y, x]) for k in range(D) if abs(k - k0) > 1]
        assert int(want[y, x]) == (min(far) if far else uo.ABSENT)


def test_small_plane_counts_and_a_flat_curve():
    rng = np.random.default_rng(22)
    C2 = rng.integers(0, 1000, (2, 7, 9))
    assert (uo.runner_up(C2) == uo.ABSENT).all() and (uo.runner_up_top4(C2)[0] == uo.ABSENT).all()
    C3 = rng.integers(0, 5, (3, 11, 13))                            # few values: ties, and every plane wins somewhere
    ks = np.argmin(C3, axis=0)
    assert set(np.unique(ks)) == {0, 1, 2}
    r3 = uo.runner_up(C3)
    assert np.array_equal(r3 == uo.ABSENT, ks == 1) and np.array_equal(uo.runner_up_top4(C3)[0], r3)
    assert np.array_equal(r3[ks == 0], C3[2][ks == 0]) and np.array_equal(r3[ks == 2], C3[0][ks == 2])
    C4 = rng.integers(0, 5, (4, 11, 13))
    assert not (uo.runner_up(C4) == uo.ABSENT).any() and np.array_equal(uo.runner_up_top4(C4)[0], uo.runner_up(C4))
    for value in (0, 37):                                           # a flat curve: C2 = C1, failing every u > 0
        flat = np.full((12, 3, 4), value, np.int64)
        r = uo.runner_up(flat)
        assert (r == value).all() and uo.unique_pass(flat[0], r, 0).all()
        assert not any(uo.unique_pass(flat[0], r, u).any() for u in (1, 5, 100))
    # the inequality in integers, at its edge: (C2 - C1) 100 >= u C2
    c1, c2 = np.array([[95, 96, 0, 7]], np.uint32), np.array([[100, 100, 1, uo.ABSENT]], np.uint32)
    assert uo.unique_pass(c1, c2, 5).tolist() == [[True, False, True, True]]
    assert uo.unique_pass(c1, c2, 100).tolist() == [[False, False, True, True]]
    big = np.array([[0xFFFFFFFE]], np.uint32)                       # 64-bit: no wrap at the largest present value
    assert uo.unique_pass(np.array([[0]], np.uint32), big, 100).all() and not uo.unique_pass(big, big, 1).any()


def test_the_filter_at_its_ends_and_monotone_in_u():
    scene, swept, _ = us.flat_row(us.FLAT_ROWS[0])
    src = [(swept[s]["depth"], scene[s][1], scene[s][2]) for s in (1, 2)]
    fd, fp = do.geometric_filter(swept[0]["depth"], swept[0]["plane"], scene[0][1], scene[0][2], src, us.FLAT_REL_TOL, us.FLAT_MIN_AGREE)
    d0, p0 = us.flat_filter(scene, swept, 0)
    assert d0.tobytes() == fd.tobytes() and p0.tobytes() == fp.tobytes()
    kept = d0 > 0
    for u in (1, 5, 30, 60, 100):
        d, p = us.flat_filter(scene, swept, u)
        now = d > 0
        print("u", u, "kept", int(now.sum()))
        assert not (now & ~kept).any() and np.array_equal(p >= 0, now)
        assert np.array_equal(d[now].view(np.uint32), fd[now].view(np.uint32)) and np.array_equal(p[now], fp[now])
        kept = now
    assert kept.sum() < (d0 > 0).sum()


@pytest.mark.parametrize("row", us.FLAT_ROWS, ids=[r[0] for r in us.FLAT_ROWS])
def test_the_defect_and_its_cure(row):
    """Kept and wrong / kept and right over all pixels of slot 0, without the test and at u = 5: flat plane (1, 20) 76 -> 3 and
    1830 -> 1816, flat step (1, 20) 36 -> 3 and 1712 -> 1712, flat plane (2, 40) 30 -> 1 and 1886 -> 1870."""
    scene, swept, truth = us.flat_row(row)
    bad = uo.wrong(swept[0], truth, us.FLAT_PLANES, *ARGS)
    with np.errstate(invalid="ignore"):
        good = np.abs(swept[0]["inv_depth"] - truth) <= do.plane_step(*ARGS, us.FLAT_PLANES)
    patch = scene[0][0] == int(ss.FLAT)
    count = {}
    for u in (0, us.FLAT_U):
        kept = us.flat_filter(scene, swept, u)[0] > 0
        count[u] = (int((kept & bad).sum()), int((kept & good).sum()))
        print(row[0], "u", u, "kept and wrong", count[u][0], "of them inside the patch", int((kept & bad & patch).sum()),
              "kept and right", count[u][1])
    assert count[0][0] >= 25                                        # the scene shows the defect
    assert 5 * count[us.FLAT_U][0] <= count[0][0]
    assert 100 * count[us.FLAT_U][1] >= 98 * count[0][1]
    table = {"flat_plane_r1_t20": ((76, 1830), (3, 1816)), "flat_step_r1_t20": ((36, 1712), (3, 1712)),
             "flat_plane_r2_t40": ((30, 1886), (1, 1870))}
    assert (count[0], count[us.FLAT_U]) == table[row[0]]


@pytest.mark.parametrize("make", [ss.flat_plane_scene, ss.flat_step_scene], ids=["flat_plane", "flat_step"])
def test_aggregated_sweeps_are_not_hurt(make):
    """Radius 1, trunc 20, P1 and P2 of sgm_scene, 8 paths: the share of all pixels that pass u = 5 on the aggregated curve is
    100 % on the flat plane and 99.9 % on the flat step."""
    v = make()
    out = uo.sweep(*v[0], [v[1], v[2]], *ARGS, 12, 1, 20, paths=8, p1=ss.P1, p2=ss.P2)
    share = float(uo.unique_pass(out["cost"], out["runner"], 5).mean())
    print("share passing u = 5 on the aggregated curve: %.4f" % share)
    assert share >= 0.99


def test_prototype_table_covers_the_unique_section():
    import __graft_entry__ as g
    pkg = g.load_package()
    from ekf_monoslam_amd import capi, dense, fusion
    names = set(pkg.declared_symbols())
    for n in ("ekf_dense_keep_runner_up", "ekf_dense_get_runner_up", "ekf_dense_filter_unique", "ekf_dense_get_unique_profile"):
        assert n in names and n in capi._PROTOS
    assert len(capi._PROTOS["ekf_dense_filter_unique"][1]) == len(capi._PROTOS["ekf_dense_filter"][1]) + 1
    assert all(hasattr(pkg.DenseStereo, m) for m in ("keep_runner_up", "runner_up", "get_unique_profile"))
    assert inspect.signature(pkg.DenseStereo.filter).parameters["uniqueness"].default == 0
    assert inspect.signature(dense.depth_maps_from_recording).parameters["uniqueness"].default == 0
    assert pkg.DepthMap.__dataclass_fields__["runner_up"].default is None
    assert len(dense.UNIQUE_KERNELS) == 6
    for u in (-1, 101):
        with pytest.raises(ValueError):
            dense.depth_maps_from_recording("nowhere", uniqueness=u)
    assert "uniqueness" in fusion.mesh_from_recording.__doc__ and "uniqueness" in fusion.audit_recording.__doc__
