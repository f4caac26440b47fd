"""Bundle adjustment of the key-frame map on the GPU: the reference's `sba_add` step.

`BundleAdjuster` binds one `ekf_sba` handle (include/ekf_monoslam.h): fp64 Levenberg-Marquardt on the reduced camera
system, node 0 fixed, as SysSBA::doSBA (sparse_bundle_adjustment/src/sba.cpp:1312-1585).  `sba_add` is the driver
(sba_add.cpp:71-290) over the three files the filter's node writes (`formats`), with the deviations of DESIGN.md
§11.4.  The pseudo-Huber cost (SysSBA::huber) and the pruning of outlying projections (countBad, removeBad,
reduceTracks) are there as well, off by default.  The linear solver is the dense Cholesky by default;
`solver="pcg"` is the reference's block-Jacobi preconditioned conjugate gradient (SBA_BLOCK_JACOBIAN_PCG, DESIGN.md
§11.7), which holds no dense matrix and has no 1024-node limit.  There is no CPU fallback: without a HIP device the
constructor raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os

import numpy as np

from . import formats
from .capi import Handle, ptr as _ptr

REFERENCE_SBA_CAMERA = (2217.0187, 2217.0187, 1280.5, 960.5)     # sba_add.cpp:206-211 (fx, fy, cx, cy)
SOLVERS = {"cholesky": 0, "pcg": 3}                              # doSBA's useCSparse (SBA_BLOCK_JACOBIAN_PCG = 3)


class SbaCamera(C.Structure):
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double)]


class BundleAdjuster(Handle):
    """One bundle-adjustment problem on the GPU (SysSBA restricted to what sba_add uses)."""
    _family = "ekf_sba"

    def __init__(self, camera=REFERENCE_SBA_CAMERA, capacity_nodes=256, capacity_points=65536,
                 capacity_projections=262144, device=0, solver="cholesky", cg_tol=1e-8, cg_max_iters=100):
        if solver not in SOLVERS:
            raise ValueError("solver must be 'cholesky' or 'pcg'")
        cam = SbaCamera(*[float(c) for c in camera])
        caps = (C.byref(cam), int(capacity_nodes), int(capacity_points), int(capacity_projections), int(device))
        if solver == "cholesky":
            self._create("ekf_sba_create", *caps)
        else:
            self._create("ekf_sba_create_solver", *caps, SOLVERS[solver])
        self.camera = tuple(float(c) for c in camera)
        self.set_cg(cg_tol, cg_max_iters)

    # --- building ---------------------------------------------------------------------------------------
    def add_nodes(self, pose7):
        """Rows (x y z qw qx qy qz); returns the index of the first new node."""
        a = np.ascontiguousarray(np.asarray(pose7, dtype=np.float64).reshape(-1, 7))
        first = self.counts()[0]
        self._check(self._lib.ekf_sba_add_nodes(self._h, a.shape[0], _ptr(a)))
        return first

    def add_points(self, xyz):
        a = np.ascontiguousarray(np.asarray(xyz, dtype=np.float64).reshape(-1, 3))
        first = self.counts()[1]
        self._check(self._lib.ekf_sba_add_points(self._h, a.shape[0], _ptr(a)))
        return first

    def add_projections(self, node, point, uv):
        """Returns the number of new (node, point) pairs (a repeat keeps the first keypoint)."""
        n = np.ascontiguousarray(np.asarray(node, dtype=np.int32).reshape(-1))
        p = np.ascontiguousarray(np.asarray(point, dtype=np.int32).reshape(-1))
        m = np.ascontiguousarray(np.asarray(uv, dtype=np.float64).reshape(-1, 2))
        if not (n.size == p.size == m.shape[0]):
            raise ValueError("node, point and uv must have the same length")
        added = C.c_int()
        self._check(self._lib.ekf_sba_add_projections(self._h, n.size, _ptr(n), _ptr(p), _ptr(m), C.byref(added)))
        return added.value

    def counts(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._check(self._lib.ekf_sba_counts(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def projections(self):
        """The stored projections, point-major and node ascending within a point: (node, point, uv, valid)."""
        n = C.c_int()
        self._check(self._lib.ekf_sba_get_projections(self._h, 0, None, None, None, None, C.byref(n)))
        node, point = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        uv, valid = np.zeros((n.value, 2)), np.zeros(n.value, np.uint8)
        self._check(self._lib.ekf_sba_get_projections(self._h, n.value, _ptr(node), _ptr(point), _ptr(uv), _ptr(valid),
                                                      C.byref(n)))
        return node, point, uv, valid.astype(bool)

    # --- robust cost and pruning ------------------------------------------------------
    @property
    def huber(self):
        """SysSBA::huber in pixels (proj.cpp:162-176); 0 (the default) is the plain squared error."""
        h = C.c_double()
        self._check(self._lib.ekf_sba_get_huber(self._h, C.byref(h)))
        return h.value

    @huber.setter
    def huber(self, value):
        self._check(self._lib.ekf_sba_set_huber(self._h, float(value)))

    def count_bad(self, dist):
        """countBad: valid projections whose weighted squared error at the current state is >= dist^2."""
        n = C.c_int()
        self._check(self._lib.ekf_sba_count_bad(self._h, float(dist), C.byref(n)))
        return n.value

    def remove_bad(self, dist):
        """removeBad: marks those projections invalid; returns how many."""
        n = C.c_int()
        self._check(self._lib.ekf_sba_remove_bad(self._h, float(dist), C.byref(n)))
        return n.value

    def reduce_tracks(self):
        """reduceTracks: erases invalid projections and the tracks left with fewer than 2; returns the points cleared."""
        n = C.c_int()
        self._check(self._lib.ekf_sba_reduce_tracks(self._h, C.byref(n)))
        return n.value

    def num_bad_points(self):
        """numBadPoints: valid projections with an exactly zero error (the point is not in front of the camera)."""
        n = C.c_int()
        self._check(self._lib.ekf_sba_num_bad_points(self._h, C.byref(n)))
        return n.value

    def avg_error(self):
        """calcAvgError: mean weighted |e| over the valid projections (NaN without any)."""
        a = C.c_double()
        self._check(self._lib.ekf_sba_avg_error(self._h, C.byref(a)))
        return a.value

    # --- linear solver ----------------------------------------------------------------
    @property
    def solver(self):
        """"cholesky" or "pcg", fixed when the handle is made."""
        v = C.c_int()
        self._check(self._lib.ekf_sba_get_solver(self._h, C.byref(v)))
        return {n: k for k, n in SOLVERS.items()}[v.value]

    def set_cg(self, tol=1e-8, max_iters=100):
        """doSBA's initTol and maxCGiters (sba.h:158-159); stored and ignored by the Cholesky solver."""
        self._check(self._lib.ekf_sba_set_cg(self._h, float(tol), int(max_iters)))

    def get_cg(self):
        t, m = C.c_double(), C.c_int()
        self._check(self._lib.ekf_sba_get_cg(self._h, C.byref(t), C.byref(m)))
        return t.value, m.value

    def cg_log(self):
        """Per LM iteration of the last run: (CG iterations, the r.s that ended the loop, the bound d0); empty for
        the Cholesky solver."""
        n = C.c_int()
        self._check(self._lib.ekf_sba_get_cg_log(self._h, 0, None, None, None, C.byref(n)))
        it, dn, d0 = np.zeros(n.value, np.int32), np.zeros(n.value), np.zeros(n.value)
        self._check(self._lib.ekf_sba_get_cg_log(self._h, n.value, _ptr(it), _ptr(dn), _ptr(d0), C.byref(n)))
        return it, dn, d0

    # --- solving --------------------------------------------------------------------------------------------
    def run(self, niter=10, lam=1e-4):
        """SysSBA::doSBA(niter, lam): the iteration count, -1 for an empty problem."""
        it = C.c_int()
        self._check(self._lib.ekf_sba_run(self._h, int(niter), float(lam), C.byref(it)))
        return it.value

    def cost(self, dist=10000.0):
        """(calcCost, calcRMSCost(dist))."""
        sq, rms = C.c_double(), C.c_double()
        self._check(self._lib.ekf_sba_cost(self._h, float(dist), C.byref(sq), C.byref(rms)))
        return sq.value, rms.value

    def rms_cost(self, dist=10000.0):
        return self.cost(dist)[1]

    def nodes(self):
        out = np.zeros((self.counts()[0], 7))
        self._check(self._lib.ekf_sba_get_nodes(self._h, _ptr(out)))
        return out

    def points(self):
        out = np.zeros((self.counts()[1], 3))
        self._check(self._lib.ekf_sba_get_points(self._h, _ptr(out)))
        return out

    def log(self):
        """Per iteration of the last run: cost before, cost after, lambda after, accepted, |x|^2."""
        n = C.c_int()
        self._check(self._lib.ekf_sba_get_log(self._h, 0, None, C.byref(n)))
        out = np.zeros((n.value, 5))
        self._check(self._lib.ekf_sba_get_log(self._h, n.value, _ptr(out), C.byref(n)))
        return out

    def profile(self, enable=True):
        self._check(self._lib.ekf_sba_profile(self._h, 1 if enable else 0))

    def get_profile(self):
        """(ms per phase: prep, Schur, assemble, factor + solve, update + cost; ms per iteration)."""
        ph = np.zeros(5)
        n = C.c_int()
        self._check(self._lib.ekf_sba_get_profile(self._h, _ptr(ph), 0, None, C.byref(n)))
        it = np.zeros(n.value)
        self._check(self._lib.ekf_sba_get_profile(self._h, _ptr(ph), n.value, _ptr(it), C.byref(n)))
        return ph, it

    def rms_wrapper(self):
        """SBANode::doSBA (sba_add.cpp:259-290): doSBA(10, 1e-4), and more while the RMS stays above 4 px."""
        if self.counts()[0] == 0:
            return
        self.run(10, 1e-4)
        c = self.rms_cost()
        if math.isnan(c) or math.isinf(c):
            return
        if self.rms_cost() > 4.0:
            self.run(10, 1e-4)
        if self.rms_cost() > 4.0:
            self.run(15, 1e-4)

    def rms_wrapper_pruned(self, prune_dist=None):
        """The RMS wrapper, then (with `prune_dist`) remove_bad(prune_dist); if that removed anything,
        reduce_tracks() and one more run(10, 1e-4).  The pruning is not part of the reference driver."""
        self.rms_wrapper()
        if prune_dist is not None and self.counts()[0] and self.remove_bad(prune_dist):
            self.reduce_tracks()
            self.run(10, 1e-4)


def sba_add(points, nodes_and_prjcts, cams_cov=None, camera=REFERENCE_SBA_CAMERA, every=10, points_out=None,
            nodes_out=None, device=0, huber=0.0, prune_dist=None, solver="cholesky", cg_tol=1e-8, cg_max_iters=100):
    """The reference's sba_add driver on the GPU.

    `points`, `nodes_and_prjcts`, `cams_cov`: paths or file objects of the filter's three files (formats.py), or
    already parsed values (an N x 12 table; a list of (id, pose7, projections); cams_cov is read for its shape
    only -- the reference computes projection covariances from it but never uses them, usecovariance = false).
    Node and point values pass through float32, as sba_add reads them (sba_add.cpp:83-86).  After every `every`-th
    node and once at the end the RMS wrapper runs.  Deviations: points.txt row 0 is an ordinary
    point, a `0  0  0` projection line means no projection, `P0` is a node id.

    Limit of the default solver (deviation 4): at most 1024 key-frame records, the largest reduced
    system the single-workgroup triangular solve holds; more raise EkfError (EKF_ERR_ARG) when the handle is created.
    `solver="pcg"` has no such limit; `cg_tol` and `cg_max_iters` are doSBA's initTol and maxCGiters.

    `camera` is (fx, fy, cx, cy) or the ``camera.txt`` a rectifying ``KeyframeRecorder`` wrote beside the three files
    (DESIGN.md §14): its rows are undistorted, so the pinhole model of the adjuster fits them.

    `huber` (pixels) is set on the handle before the first run (SysSBA::huber; the reference driver leaves it 0).
    With `prune_dist` every call of the RMS wrapper is followed by remove_bad(prune_dist) and, if that removed
    anything, reduce_tracks() and one more run(10, 1e-4).  The reference driver has no such option (the library
    calls exist, sba_add.cpp never makes them); the defaults reproduce it exactly.

    Returns (table, nodes, ids): the refined N x 3 table (rows of points that were never added -- all-zero ones --
    stay zero), the refined nodes (x y z qw qx qy qz) and their ids.  Writes Points_Out.txt / Nodes_Out.txt when
    `points_out` / `nodes_out` are given.
    """
    if isinstance(camera, (str, os.PathLike)) or hasattr(camera, "read"):
        camera = formats.read_camera(camera)
    table = points if isinstance(points, np.ndarray) else formats.read_points(points)
    table = np.asarray(table, dtype=np.float32)
    records = nodes_and_prjcts if isinstance(nodes_and_prjcts, list) else formats.read_pose_records(nodes_and_prjcts)
    if cams_cov is not None and not isinstance(cams_cov, np.ndarray):
        formats.read_camera_covs(cams_cov)
    rows = [i for i in range(table.shape[0]) if table[i, 0] or table[i, 1] or table[i, 2]]
    row_of = {r: k for k, r in enumerate(rows)}
    nproj = sum(len(r[2]) for r in records)
    ba = BundleAdjuster(camera, capacity_nodes=max(len(records), 1), capacity_points=max(len(rows), 1),
                        capacity_projections=max(nproj, 1), device=device, solver=solver, cg_tol=cg_tol,
                        cg_max_iters=cg_max_iters)
    ba.huber = huber
    if rows:
        ba.add_points(table[rows, :3].astype(np.float64))
    ids = []
    for pid, pose, prj in records:
        ni = ba.add_nodes(np.asarray(pose, dtype=np.float32).astype(np.float64).reshape(1, 7))
        ids.append(int(pid))
        sel = [(row_of[int(ri)], float(int(u)), float(int(v))) for ri, u, v in np.asarray(prj).reshape(-1, 3)
               if not (ri == 0 and u == 0 and v == 0) and int(ri) in row_of]
        if sel:
            s = np.array(sel)
            ba.add_projections(np.full(len(sel), ni), s[:, 0].astype(np.int32), s[:, 1:])
        if every and (ni + 1) % every == 0:
            ba.rms_wrapper_pruned(prune_dist)
    ba.rms_wrapper_pruned(prune_dist)
    out = np.zeros((table.shape[0], 3))
    if rows:
        out[rows] = ba.points()
    nodes = ba.nodes()
    if points_out is not None:
        formats.write_points_out(points_out, ba.points())
    if nodes_out is not None:
        formats.write_nodes_out(nodes_out, ids, nodes)
    ba.close()
    return out, nodes, ids
