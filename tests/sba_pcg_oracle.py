"""numpy restatement of the reference's block-Jacobi PCG solve on top of tests/sba_oracle.py.

Paths are under sparse_bundle_adjustment/.  doSBA(niter, lambda, useCSparse = SBA_BLOCK_JACOBIAN_PCG, initTol,
maxCGiters) (sba.cpp:1312, :1417-1421) keeps the Schur-reduced camera system as 6 x 6 blocks -- `diag` and, per block
column, the upper off-diagonal blocks `cols` (CSparse::setupBlockStructure / addOffdiagBlock / incDiagBlocks;
setupSparseSys, sba.cpp:1165-1302) -- and solves it with CSparse::doBPCG (csparse.cpp:383-395):

- jacobiBPCG<6>::doBPCG2 (bpcg/bpcg.h:238-316): x = 0, r = b, d = J r with J_i = diag_i^-1, dn = r.d, d0 = tol dn;
  when `abstol` is set (sba_iter > 0, csparse.cpp:390) d0 is raised to `residual`, which the solve before left at dn / 2
  (bpcg.h:314) and which lives as long as the system object.  Up to maxCGiters times: stop if dn < d0; q = A d;
  a = dn / d.q; x += a d; r -= a q; s = J r; dold = dn; dn = r.s; d = s + (dn / dold) d.  The result replaces B.
- jacobiBPCG::mMV2 (bpcg.h:142-161): vout_i = diag_i vin_i for every i, then over the off-diagonal entries in storage
  order (block column ascending, block row ascending within it), for the block M at block row ri, block column ii:
  vout_ri += M vin_ii, then vout_ii += M^T vin_ri.  For one block row that is: its neighbours in ascending order.

The system itself is sba_oracle's (and sba_robust_oracle's, when the class is built on RobustSysSBA): the same sums in
the same order, kept per block instead of in a dense matrix, so that a problem with thousands of nodes fits.
`dtype` (float64 or numpy.longdouble) is the arithmetic of the CG alone; the system is always built in float64.

Deviations carried over (DESIGN.md §11.4 no 1 and 2, §11.6 no 2): a free node without a valid projection gets the
identity block and a zero right-hand side; a diagonal block that is not positive definite raises NotPositiveDefinite
(the reference inverts whatever it finds).
"""
from __future__ import annotations

import numpy as np

import sba_oracle as so
import sba_robust_oracle as ro


class BlockSystem:
    """diag: (nfree, 6, 6); off: {(a, b): 6 x 6 block at block row a, block column b, a < b}."""

    def __init__(self, diag, off):
        self.diag = diag
        self.off = off

    def to_dense(self):
        n = len(self.diag)
        A = np.zeros((6 * n, 6 * n))
        for i in range(n):
            A[6 * i:6 * i + 6, 6 * i:6 * i + 6] = self.diag[i]
        for (a, b), M in self.off.items():
            A[6 * a:6 * a + 6, 6 * b:6 * b + 6] = M
            A[6 * b:6 * b + 6, 6 * a:6 * a + 6] = M.T
        return A

    def entries(self):
        """mMV2's linear storage (bpcg.h:259-276): block columns ascending, block rows ascending within a column."""
        keys = sorted(self.off, key=lambda k: (k[1], k[0]))
        rind = np.array([k[0] for k in keys], dtype=np.int64)
        cind = np.array([k[1] for k in keys], dtype=np.int64)
        M = np.array([self.off[k] for k in keys]).reshape(-1, 6, 6)
        return rind, cind, M


class _BlockPcg:
    """Mix-in in front of SysSBA / RobustSysSBA: block assembly, doBPCG2 as `solve`, the residual carry-over."""

    cg_tol = 1e-8          # doSBA's initTol (sba.h:158-159)
    cg_max = 100           # doSBA's maxCGiters
    dtype = np.float64     # arithmetic of the CG

    def set_cg(self, tol=1e-8, max_iters=100, dtype=np.float64):
        self.cg_tol, self.cg_max, self.dtype = float(tol), int(max_iters), dtype
        return self

    # jacobiBPCG::residual and the per-solve log: (CG iterations, final dn, d0, dn before the first iteration)
    residual = 0.0
    cg_log = ()
    _sba_iter = 0

    def _track_nodes(self, pi):
        return self._valid_nodes(pi) if hasattr(self, "valid") else sorted(self.tracks[pi])

    def setup_sparse_sys(self, lam_in):
        """setupSparseSys + the diagonal scaling, per block.  Returns (BlockSystem, B, tps, Tpc)."""
        nn = len(self.trans)
        nfree = max(nn - 1, 0)
        huber = getattr(self, "huber", 0.0)
        m = self._mats()
        lam = 1.0 + lam_in
        diag = np.zeros((nfree, 6, 6))
        off = {}
        B = np.zeros(6 * nfree)
        tps = [np.zeros(3) for _ in self.points]
        Tpc = {}
        seen = set()
        for pi, tr in enumerate(self.tracks):
            nodes = self._track_nodes(pi)
            if not nodes:
                continue
            seen.update(nodes)
            X = self.points[pi]
            Hpp = np.zeros((3, 3))
            bp = np.zeros(3)
            jp = {}
            for ni in nodes:
                w2n, w2i, dR = m[ni]
                e, _ = ro.proj_error(w2i, X, tr[ni], huber)
                jacc, jacp = so.proj_jacobians(w2n, dR, self.trans[ni], X, self.camera)
                jp[ni] = dict(Hpp=jacp.T @ jacp, Hcc=jacc.T @ jacc, Hpc=jacp.T @ jacc, JcTE=jacc.T @ e, Bp=jacp.T @ e)
                Hpp = Hpp + jp[ni]["Hpp"]
                bp = bp - jp[ni]["Bp"]
                if ni >= 1:
                    diag[ni - 1] += jp[ni]["Hcc"]
                    B[6 * (ni - 1):6 * ni] -= jp[ni]["JcTE"]
            Hpp[np.diag_indices(3)] *= lam
            Hppi = so.inv3(Hpp)
            tp = Hppi @ bp
            tps[pi] = tp
            free = [ni for ni in nodes if ni >= 1]
            for k, ni in enumerate(free):
                B[6 * (ni - 1):6 * ni] -= jp[ni]["Hpc"].T @ tp
                T = jp[ni]["Hpc"].T @ Hppi
                Tpc[(pi, ni)] = T
                for ni2 in free[k:]:
                    blk = -(T @ jp[ni2]["Hpc"])
                    if ni2 == ni:
                        diag[ni - 1] += blk
                    else:
                        key = (ni - 1, ni2 - 1)
                        off[key] = off.get(key, np.zeros((6, 6))) + blk
        iu = np.triu_indices(6, 1)
        for i in range(nfree):
            diag[i].T[iu] = diag[i][iu]                  # the reference keeps the upper triangle of a diagonal block
            diag[i][np.diag_indices(6)] *= lam
        for ni in range(1, nn):                          # deviation 1: a free node without a valid projection
            if ni not in seen:
                diag[ni - 1] = np.eye(6)
                B[6 * (ni - 1):6 * ni] = 0.0
        return BlockSystem(diag, off), B, tps, Tpc

    def solve(self, A, B):
        """CSparse::doBPCG: doBPCG2 from x = 0 with abstol from the second LM iteration of a run on."""
        T = self.dtype
        n = len(A.diag)
        try:
            for D in A.diag:
                np.linalg.cholesky(D)
        except np.linalg.LinAlgError as exc:
            raise so.NotPositiveDefinite(str(exc)) from None
        if not np.isfinite(A.diag).all():
            raise so.NotPositiveDefinite("a diagonal block is not finite")
        J = np.linalg.inv(A.diag).astype(T)
        Dg = A.diag.astype(T)
        rind, cind, M = A.entries()
        M = M.astype(T)
        idx = np.empty(2 * len(rind), dtype=np.int64)
        idx[0::2], idx[1::2] = rind, cind

        def mmv(v):
            out = np.einsum("nij,nj->ni", Dg, v)
            if len(rind):
                contrib = np.empty((2 * len(rind), 6), dtype=T)
                contrib[0::2] = np.einsum("eij,ej->ei", M, v[cind])      # vout_ri += M vin_ii
                contrib[1::2] = np.einsum("eji,ej->ei", M, v[rind])      # vout_ii += M^T vin_ri
                np.add.at(out, idx, contrib)                              # unbuffered: in entry order
            return out

        def md(v):
            return np.einsum("nij,nj->ni", J, v)

        def dot(u, v):
            return np.dot(u.reshape(-1), v.reshape(-1))

        abstol = self._sba_iter > 0
        self._sba_iter += 1
        x = np.zeros((n, 6), dtype=T)
        r = B.astype(T).reshape(n, 6).copy()
        d = md(r)
        dn = dot(r, d)
        dn0 = dn
        d0 = T(self.cg_tol) * dn
        if abstol and self.residual > d0:
            d0 = T(self.residual)
        i = 0
        while i < self.cg_max:
            if dn < d0:
                break
            q = mmv(d)
            a = dn / dot(d, q)
            x = x + a * d
            r = r - a * q
            s = md(r)
            dold = dn
            dn = dot(r, s)
            d = s + (dn / dold) * d
            i += 1
        self.residual = dn / T(2.0)
        if not isinstance(self.cg_log, list):
            self.cg_log = []
        self.cg_log.append((i, float(dn), float(d0), float(dn0)))
        return x.reshape(-1).astype(np.float64)

    def do_sba(self, niter, s_lambda=-1.0):
        self._sba_iter = 0
        self.cg_log = []
        return super().do_sba(niter, s_lambda)


class PcgSysSBA(_BlockPcg, so.SysSBA):
    """sba_oracle.SysSBA with doSBA's useCSparse = SBA_BLOCK_JACOBIAN_PCG."""


class RobustPcgSysSBA(_BlockPcg, ro.RobustSysSBA):
    """sba_robust_oracle.RobustSysSBA (huber, validity flags, pruning) with the PCG solve."""


def pcg_system(scene, huber=None):
    """The oracle of a sba_scene / sba_robust_scene scene; `huber` not None gives the robust class."""
    s = PcgSysSBA(scene["camera"]) if huber is None else RobustPcgSysSBA(scene["camera"], huber)
    for p in scene["nodes"]:
        s.add_node(p)
    for x in scene["points"]:
        s.add_point(x)
    for ni, pi, m in zip(scene["node"], scene["point"], scene["uv"]):
        s.add_proj(int(ni), int(pi), m)
    return s
