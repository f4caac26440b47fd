"""CPU checks of the block-Jacobi PCG oracle (tests/sba_pcg_oracle.py) and of the argument checks of the
new ekf_sba_* entry points that need no device."""
import ctypes as C

import numpy as np
import pytest

import sba_oracle as so
import sba_pcg_oracle as po
import sba_scene as sc


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return g.load_package()


def test_block_system_is_the_dense_system():
    scene = sc.make_scene(4, 60, seed=8)                         # the last node has no projection: identity block
    A, B, tps, _ = po.pcg_system(scene).setup_sparse_sys(1e-4)
    A2, B2, tps2, _ = sc.oracle_system(scene).setup_sparse_sys(1e-4)
    assert np.array_equal(A.to_dense(), A2) and np.array_equal(B, B2)
    assert all(np.array_equal(a, b) for a, b in zip(tps, tps2))
    assert np.array_equal(A.diag[-1], np.eye(6)) and not B[-6:].any()
    assert all(a < b for a, b in A.off)                          # upper blocks only
    rind, cind, _ = A.entries()
    assert list(zip(cind, rind)) == sorted(zip(cind, rind))      # block column, then block row


def test_converged_cg_is_the_dense_solve():
    scene = sc.make_scene(5, 120, seed=2)
    for T in (np.float64, np.longdouble):
        s = po.pcg_system(scene).set_cg(1e-30, 1000, dtype=T)
        A, B, _, _ = s.setup_sparse_sys(1e-4)
        x = s.solve(A, B)
        x_ref = so.SysSBA.solve(A.to_dense(), B)
        it, dn, d0, dn0 = s.cg_log[-1]
        assert it < 1000 and dn < d0 and d0 == 1e-30 * dn0
        assert np.abs(x - x_ref).max() <= 1e-9 * np.abs(x_ref).max()
        assert s.residual == pytest.approx(dn / 2.0)


def test_mat_vec_order_is_neighbours_ascending():
    """mMV2's entry order gives, for each block row, D_i d_i and then its neighbours in ascending order."""
    scene = sc.make_scene(6, 150, seed=3, lonely_node=False)
    A, _, _, _ = po.pcg_system(scene).setup_sparse_sys(1e-4)
    rind, cind, M = A.entries()
    rng = np.random.default_rng(0)
    v = rng.normal(size=(len(A.diag), 6))
    out = np.einsum("nij,nj->ni", A.diag, v)
    for ri, ii, m in zip(rind, cind, M):                         # bpcg.h:153-160, literally
        out[ri] += m @ v[ii]
        out[ii] += m.T @ v[ri]
    rows = np.einsum("nij,nj->ni", A.diag, v)
    for i in range(len(A.diag)):
        for nb in sorted({b for a, b in A.off if a == i} | {a for a, b in A.off if b == i}):
            rows[i] += A.off[(i, nb)] @ v[nb] if nb > i else A.off[(nb, i)].T @ v[i * 0 + nb]
    assert np.array_equal(out, rows)


def test_truncated_cg_and_abstol_rule():
    scene = sc.make_scene(11, 300, seed=0)
    s = po.pcg_system(scene)
    assert (s.cg_tol, s.cg_max) == (1e-8, 100)                   # sba.h:158-159
    assert s.do_sba(3, 1e-4) == 3
    (i0, dn_0, d0_0, dn0_0), (i1, dn_1, d0_1, dn0_1), (i2, dn_2, d0_2, dn0_2) = s.cg_log
    assert i0 == 51 and d0_0 == 1e-8 * dn0_0                      # first LM iteration: relative bound only
    assert d0_1 == max(1e-8 * dn0_1, dn_0 / 2.0) and d0_2 == max(1e-8 * dn0_2, dn_1 / 2.0)
    assert d0_1 == dn_0 / 2.0                                     # here the carried residual is the larger one
    assert s.residual == dn_2 / 2.0
    s.do_sba(1, 0.0)                                              # a new run: sba_iter = 0, no carry-over
    assert s.cg_log[0][2] == 1e-8 * s.cg_log[0][3]
    # an inexact solve is not an error: one CG iteration per solve still runs, LM accepts or rejects
    t = po.pcg_system(scene).set_cg(1e-8, 1)
    assert t.do_sba(3, 1e-4) == 3 and [l[0] for l in t.cg_log] == [1, 1, 1]


def test_robust_class_uses_weights_and_flags():
    import sba_robust_scene as rs
    scene = rs.make_robust_scene(5, 120, seed=5)
    s = po.pcg_system(scene, 2.0)
    c = rs.oracle_system(scene, 2.0)
    for o in (s, c):
        o.remove_bad(60.0)
    A, B, _, _ = s.setup_sparse_sys(1e-4)
    A2, B2, _, _ = c.setup_sparse_sys(1e-4)
    assert np.array_equal(A.to_dense(), A2) and np.array_equal(B, B2)


def test_not_positive_definite_block_raises():
    s = po.PcgSysSBA()
    D = np.eye(6)
    D[2, 2] = -1.0
    with pytest.raises(so.NotPositiveDefinite):
        s.solve(po.BlockSystem(np.array([D]), {}), np.ones(6))


def test_prototypes_and_constants(pkg):
    from ekf_monoslam_amd import capi, sba
    for name in ("ekf_sba_create_solver", "ekf_sba_get_solver", "ekf_sba_set_cg", "ekf_sba_get_cg",
                 "ekf_sba_get_cg_log"):
        assert name in capi._PROTOS and name in pkg.declared_symbols()
        assert hasattr(pkg.load_library(), name)
    assert sba.SOLVERS == {"cholesky": 0, "pcg": 3}              # SBA_BLOCK_JACOBIAN_PCG = 3
    header = open(capi.HEADER_PATH).read()
    assert "#define EKF_SBA_SOLVER_CHOLESKY 0" in header and "#define EKF_SBA_SOLVER_BPCG 3" in header


def test_abi_checks_without_a_device(pkg):
    import torch
    lib = pkg.load_library()
    h = C.c_void_p()
    good = pkg.sba.SbaCamera(*sc.CAMERA)
    bad = pkg.sba.SbaCamera(-1.0, 500.0, 320.0, 240.0)
    for solver in (1, 2, 4, -1):                                  # SBA_GRADIENT (2) included
        assert lib.ekf_sba_create_solver(C.byref(good), 10, 10, 10, 0, solver, C.byref(h)) == 1
        assert b"solver" in lib.ekf_sba_last_error(None)
    assert lib.ekf_sba_create_solver(C.byref(bad), 10, 10, 10, 0, 3, C.byref(h)) == 1
    assert b"bad argument" in lib.ekf_sba_last_error(None)
    assert lib.ekf_sba_create_solver(C.byref(good), 2000, 10, 10, 0, 0, C.byref(h)) == 1     # solver 0 keeps the cap
    assert b"1024" in lib.ekf_sba_last_error(None)
    assert lib.ekf_sba_create_solver(C.byref(good), 0, 10, 10, 0, 3, C.byref(h)) == 1
    assert lib.ekf_sba_create_solver(C.byref(good), 2 ** 31 - 1, 10, 10, 0, 3, C.byref(h)) == 1
    assert lib.ekf_sba_create_solver(C.byref(good), 10, 10, 10, 0, 3, None) == 1
    assert lib.ekf_sba_set_cg(None, 1e-8, 100) == 1
    assert lib.ekf_sba_get_cg(None, None, None) == 1
    assert lib.ekf_sba_get_solver(None, None) == 1
    assert lib.ekf_sba_get_cg_log(None, 0, None, None, None, None) == 1
    rc = lib.ekf_sba_create_solver(C.byref(good), 2000, 10, 10, 0, 3, C.byref(h))            # beyond 1024: PCG takes it
    if torch.cuda.is_available():
        assert rc == 0
        lib.ekf_sba_destroy(h)
    else:
        assert rc == 3 and b"no CPU fallback" in lib.ekf_sba_last_error(None)                # EKF_ERR_DEVICE
    with pytest.raises(ValueError):
        pkg.BundleAdjuster(solver="gradient")
