"""numpy fp64 restatement of the reference's robust bundle adjustment on top of tests/sba_oracle.py.

Paths are under sparse_bundle_adjustment/.  What this adds to `sba_oracle.SysSBA`:

- SysSBA::huber (sba.h:113): calcErrMono_'s pseudo-Huber weight (proj.cpp:162-176), passed by calcCost(),
  calcRMSCost() and calcAvgError() (sba.cpp:300, :350, :378).  setJacobians reuses the error the last calcCost() left in
  the projection, and doSBA always calls calcCost() at the state the system is then built for (sba.cpp:1365, :1528,
  :1568), so the weighted error is what enters JcTE and bp.  The Jacobian products are not weighted.
- Proj::isValid: one flag per stored projection, set on add.  Every loop of setupSparseSys, the costs and the update
  skips an invalid projection (sba.cpp:299, :1212, :1242, :1255, :1513); it still occupies its map entry.
- countBad, removeBad, reduceTracks, numBadPoints, calcAvgError (sba.cpp:365-502).  countBad / removeBad read the error
  the last cost call stored; here they evaluate the weighted error at the current state, which is what doSBA leaves.
  (countBad's `#ifdef HUBER` rescaling of dist is compiled out in the reference and is not restated.)

Loop order everywhere: points ascending, nodes ascending within a point, as the reference's tracks and their maps.

Deviations, on top of the two of sba_oracle.py:
1. a point whose projections are all invalid is skipped like a point without projections (the reference would invert
   a zero Hpp and write NaN into the point);
2. a free node whose projections are all invalid gets the identity block of deviation 1 of §11.4: its step is 0.
"""
from __future__ import annotations

import math

import numpy as np

import sba_oracle as so


def huber_weight(e, huber):
    """proj.cpp:166-176 on an error (2,): returns (weighted error, its squared norm)."""
    e = np.asarray(e, dtype=np.float64)
    if huber > 0:
        b2 = huber * huber
        e2 = float(e @ e)
        if e2 > b2:
            c = 2.0 * huber * math.sqrt(e2) - b2
            w = math.sqrt(c / e2)
            e = e * w
    return e, float(e @ e)


def proj_error(w2i, X, kp, huber):
    """calcErrMono_ with its huber argument: p1.z <= 0 gives zero error with and without Huber."""
    e, _ = so.proj_error(w2i, X, kp)
    return huber_weight(e, huber)


class RobustSysSBA(so.SysSBA):
    """sba_oracle.SysSBA + huber, Proj::isValid and the pruning calls."""

    def __init__(self, camera=so.REFERENCE_SBA_CAMERA, huber=0.0):
        super().__init__(camera)
        self.huber = float(huber)
        self.valid = []            # per point: {node index: bool}, the keys of self.tracks[pi]

    # --- building ---------------------------------------------------------------------------------------
    def add_point(self, xyz):
        self.valid.append({})
        return super().add_point(xyz)

    def add_proj(self, ni, pi, uv):
        """addMonoProj: an invalid projection still holds its (node, point) entry and blocks a repeat."""
        new = ni not in self.tracks[pi]
        ok = super().add_proj(ni, pi, uv)
        if new:
            self.valid[pi][ni] = True
        return ok

    def _valid_nodes(self, pi):
        return [ni for ni in sorted(self.tracks[pi]) if self.valid[pi][ni]]

    def projections(self):
        """(node, point, uv, valid) of the stored projections, point-major, node ascending within a point."""
        rows = [(ni, pi, self.tracks[pi][ni], self.valid[pi][ni]) for pi in range(len(self.tracks))
                for ni in sorted(self.tracks[pi])]
        return (np.array([r[0] for r in rows], np.int32), np.array([r[1] for r in rows], np.int32),
                np.array([r[2] for r in rows], np.float64).reshape(-1, 2), np.array([r[3] for r in rows], bool))

    # --- costs --------------------------------------------------------------------------------------------
    def weighted_errors(self):
        """The weighted error vector of every valid projection, in loop order."""
        m = self._mats()
        return [proj_error(m[ni][1], self.points[pi], self.tracks[pi][ni], self.huber)[0]
                for pi in range(len(self.tracks)) for ni in self._valid_nodes(pi)]

    def errors(self):
        """Weighted squared error per valid projection (calcCost's summands, sba.cpp:289-305)."""
        return np.array([float(e @ e) for e in self.weighted_errors()], dtype=np.float64)

    def calc_avg_error(self):
        """calcAvgError (sba.cpp:365-386): 0 / 0 without a valid projection."""
        c, n = 0.0, 0
        for e in self.weighted_errors():
            c += math.sqrt(float(e @ e))
            n += 1
        return c / n if n else float("nan")

    def num_bad_points(self):
        """numBadPoints (sba.cpp:389-411): calcErr without huber, exactly zero error."""
        m = self._mats()
        n = 0
        for pi in range(len(self.tracks)):
            for ni in self._valid_nodes(pi):
                e, _ = so.proj_error(m[ni][1], self.points[pi], self.tracks[pi][ni])
                n += int(e[0] == 0.0 and e[1] == 0.0)
        return n

    # --- pruning ------------------------------------------------------------------------------------------
    def count_bad(self, dist):
        """countBad (sba.cpp:416-440)."""
        d2 = dist * dist
        return int(sum(1 for e in self.errors() if e >= d2))

    def remove_bad(self, dist):
        """removeBad (sba.cpp:445-462)."""
        d2 = dist * dist
        errs = iter(self.errors())
        n = 0
        for pi in range(len(self.tracks)):
            for ni in self._valid_nodes(pi):
                if next(errs) >= d2:
                    self.valid[pi][ni] = False
                    n += 1
        return n

    def reduce_tracks(self):
        """reduceTracks (sba.cpp:467-502): counts every track with ngood < 2, the empty ones included."""
        ret = 0
        for pi, tr in enumerate(self.tracks):
            for ni in [ni for ni in tr if not self.valid[pi][ni]]:
                del tr[ni]
                del self.valid[pi][ni]
            if len(tr) < 2:
                tr.clear()
                self.valid[pi].clear()
                ret += 1
        return ret

    # --- one linear system -------------------------------------------------------------------------------
    def setup_sparse_sys(self, lam_in):
        """sba_oracle's setup_sparse_sys over the valid projections, with the weighted error in JcTE and bp."""
        nn = len(self.trans)
        nfree = max(nn - 1, 0)
        m = self._mats()
        lam = 1.0 + lam_in
        A = np.zeros((6 * nfree, 6 * nfree))
        B = np.zeros(6 * nfree)
        tps = [np.zeros(3) for _ in self.points]
        Tpc = {}
        seen = set()
        for pi, tr in enumerate(self.tracks):
            nodes = self._valid_nodes(pi)
            if not nodes:                                   # no projection, or (deviation 1) none valid
                continue
            seen.update(nodes)
            X = self.points[pi]
            Hpp = np.zeros((3, 3))
            bp = np.zeros(3)
            jp = {}
            for ni in nodes:
                w2n, w2i, dR = m[ni]
                e, _ = proj_error(w2i, X, tr[ni], self.huber)
                jacc, jacp = so.proj_jacobians(w2n, dR, self.trans[ni], X, self.camera)
                jp[ni] = dict(Hpp=jacp.T @ jacp, Hcc=jacc.T @ jacc, Hpc=jacp.T @ jacc, JcTE=jacc.T @ e, Bp=jacp.T @ e)
                Hpp = Hpp + jp[ni]["Hpp"]
                bp = bp - jp[ni]["Bp"]
                if ni >= 1:
                    c = 6 * (ni - 1)
                    A[c:c + 6, c:c + 6] += jp[ni]["Hcc"]
                    B[c:c + 6] -= jp[ni]["JcTE"]
            Hpp[np.diag_indices(3)] *= lam
            Hppi = so.inv3(Hpp)
            tp = Hppi @ bp
            tps[pi] = tp
            free = [ni for ni in nodes if ni >= 1]
            for k, ni in enumerate(free):
                c = 6 * (ni - 1)
                B[c:c + 6] -= jp[ni]["Hpc"].T @ tp
                T = jp[ni]["Hpc"].T @ Hppi
                Tpc[(pi, ni)] = T
                for ni2 in free[k:]:
                    c2 = 6 * (ni2 - 1)
                    A[c:c + 6, c2:c2 + 6] += -(T @ jp[ni2]["Hpc"])
        iu = np.triu_indices(6 * nfree, 1)
        A.T[iu] = A[iu]
        A[np.diag_indices(6 * nfree)] *= lam
        # deviation 1 of §11.4 and deviation 2 here: a free node without a valid projection
        for ni in range(1, nn):
            if ni not in seen:
                c = 6 * (ni - 1)
                A[c:c + 6, c:c + 6] = np.eye(6)
                B[c:c + 6] = 0.0
        return A, B, tps, Tpc

    # --- the LM loop -------------------------------------------------------------------------------------
    def do_sba(self, niter, s_lambda=-1.0):
        """doSBA.  The emptiness test counts stored projections (sba.cpp:1325-1335); the loop itself, the update
        included (sba.cpp:1513), sees the valid ones only, so the base loop runs over a valid-only view of the tracks."""
        if self.nprojs == 0 or not self.points or not self.trans:
            self.log = []
            return -1
        stored, flags = self.tracks, self.valid
        self.tracks = [{ni: tr[ni] for ni in self._valid_nodes(pi)} for pi, tr in enumerate(stored)]
        self.valid = [{ni: True for ni in tr} for tr in self.tracks]
        try:
            if self.nprojs == 0:                            # nothing valid: B = 0, |x|^2 = 0 at iteration 0
                self.log = []
                if s_lambda > 0.0:
                    self.lam = s_lambda
                return 0
            return super().do_sba(niter, s_lambda)
        finally:
            self.tracks, self.valid = stored, flags

    def rms_wrapper_pruned(self, prune_dist=None):
        """The RMS wrapper, then remove_bad(prune_dist); if anything went, reduce_tracks() and one more doSBA(10, 1e-4)
        (sba.sba_add's prune_dist; not part of the reference driver)."""
        self.rms_wrapper()
        if prune_dist is not None and self.trans and self.remove_bad(prune_dist):
            self.reduce_tracks()
            self.do_sba(10, 1e-4)


def sba_add(points_table, records, camera=so.REFERENCE_SBA_CAMERA, every=10, huber=0.0, prune_dist=None):
    """sba_oracle.sba_add with `huber` set before the first run and the pruned RMS wrapper."""
    s = RobustSysSBA(camera, huber)
    pts = np.asarray(points_table, dtype=np.float32)
    row_of = {}
    rows = []
    for i in range(pts.shape[0]):
        if pts[i, 0] or pts[i, 1] or pts[i, 2]:
            row_of[i] = s.add_point(pts[i, :3].astype(np.float64))
            rows.append(i)
    ids = []
    for pid, pose, prj in records:
        ni = s.add_node(np.asarray(pose, dtype=np.float32).astype(np.float64))
        ids.append(pid)
        for ri, u, v in np.asarray(prj).reshape(-1, 3):
            if (ri, u, v) == (0, 0, 0):
                continue
            if int(ri) in row_of:
                s.add_proj(ni, row_of[int(ri)], (float(int(u)), float(int(v))))
        if every and len(s.trans) % every == 0:
            s.rms_wrapper_pruned(prune_dist)
    s.rms_wrapper_pruned(prune_dist)
    return s, rows, ids
