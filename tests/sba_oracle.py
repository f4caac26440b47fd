"""numpy fp64 restatement of the reference's sparse bundle adjustment (the `sba_add` step).

Paths are under sparse_bundle_adjustment/ unless they name mono-slam/.  Everything is fp64, as in the reference.

- Node: pose = trans (camera centre, world) + qrot (w, x, y, z), normRot() on add (node.cpp:52-66),
  w2n = [R^T | -R^T t], w2i = K w2n, dRd* = dRi* R^T (node.cpp:18-30, 96-108).  Node 0 is fixed (nFixed = 1, sba.h:85).
- Projection: addMonoProj (sba.cpp:133-143); per point the projections are a std::map keyed by node index.
- Error: calcErrMono_ (proj.cpp:143-187), no Huber (huber = 0, sba.h:86).
- Jacobians: setJacobiansMono_ (proj.cpp:60-133), local angles, qScale = 1.
- Reduced system: setupSparseSys (sba.cpp:1163-1290) + setupCSstructure's diagonal scaling (csparse.cpp:279).
- Solve: doChol, CHOLMOD branch (csparse.cpp:307-363): Cholesky, x = A^-1 B, one step of iterative refinement.
- LM loop: doSBA (sba.cpp:1312-1585).  Costs: calcCost / calcRMSCost (sba.cpp:289-360).
- Driver: SBANode::addFrame / doSBA (sba_add.cpp:71-290), with the deviations of DESIGN.md §11.4.

Deviations from the reference, restated here so that the GPU path has one thing to match:
1. a free node with no projection gets an identity diagonal block and a zero right-hand side (its step is 0);
2. any other non-positive pivot raises `NotPositiveDefinite`; nodes and points stay at the last accepted iterate.
"""
from __future__ import annotations

import math

import numpy as np

REFERENCE_SBA_CAMERA = (2217.0187, 2217.0187, 1280.5, 960.5)     # sba_add.cpp:206-211 (fx, fy, cx, cy)

# node.cpp:18-30: derivatives of the inverse rotation wrt the local-angle increment
DRI = (np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 2.0], [0.0, -2.0, 0.0]]),
       np.array([[0.0, 0.0, -2.0], [0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]),
       np.array([[0.0, 2.0, 0.0], [-2.0, 0.0, 0.0], [0.0, 0.0, 0.0]]))
SQ_MIN_DELTA = 1e-8 * 1e-8       # sba.cpp:1364


class NotPositiveDefinite(ArithmeticError):
    """Deviation 2: a non-positive pivot of the reduced camera system (not a projection-less free node)."""


def norm_rot(q):
    """Node::normRot (node.cpp:52-66) on q = (w, x, y, z)."""
    q = np.array(q, dtype=np.float64)
    v = q[1:].copy()
    if q[0] < 0:
        v = -v
    sn = float(v @ v)
    if sn >= 0.9999:
        v *= -1.0 / (math.sqrt(sn) * 1.0001)
    return np.array([math.sqrt(1.0 - float(v @ v)), v[0], v[1], v[2]])


def quat_rot(q):
    """Eigen Quaternion::toRotationMatrix for q = (w, x, y, z)."""
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def quat_mul(a, b):
    aw, ax, ay, az = a
    bw, bx, by, bz = b
    return np.array([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw])


def kmat(camera):
    fx, fy, cx, cy = camera
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def node_mats(t, q, camera):
    """(w2n, w2i, dRdx, dRdy, dRdz) of one node (transformW2F, setProjection, setDr(true))."""
    Rt = quat_rot(q).T
    w2n = np.hstack([Rt, (-Rt @ t).reshape(3, 1)])
    return w2n, kmat(camera) @ w2n, [D @ Rt for D in DRI]


def proj_error(w2i, X, kp):
    """calcErrMono_: (err(2), squared cost); p1.z <= 0 gives zero error and zero cost."""
    p1 = w2i @ np.append(X, 1.0)
    if p1[2] <= 0.0:
        return np.zeros(2), 0.0
    e = p1[:2] / p1[2] - kp
    return e, float(e @ e)


def proj_jacobians(w2n, dR, t, X, camera):
    """setJacobiansMono_: (jacc 2x6, jacp 2x3)."""
    fx, fy = camera[0], camera[1]
    pc = w2n @ np.append(X, 1.0)
    px, py, pz = pc
    ipz2 = 1.0 / (pz * pz)
    ipz2fx, ipz2fy = ipz2 * fx, ipz2 * fy
    pwt = X - t
    jacc = np.zeros((2, 6))
    jacp = np.zeros((2, 3))
    for k in range(3):
        dp = dR[k] @ pwt
        jacc[0, 3 + k] = (pz * dp[0] - px * dp[2]) * ipz2fx
        jacc[1, 3 + k] = (pz * dp[1] - py * dp[2]) * ipz2fy
    for k in range(3):
        dp = -w2n[:, k]
        jacc[0, k] = (pz * dp[0] - px * dp[2]) * ipz2fx
        jacc[1, k] = (pz * dp[1] - py * dp[2]) * ipz2fy
        dp = w2n[:, k]
        jacp[0, k] = (pz * dp[0] - px * dp[2]) * ipz2fx
        jacp[1, k] = (pz * dp[1] - py * dp[2]) * ipz2fy
    return jacc, jacp


def inv3(H):
    """Eigen's cofactor inverse of a 3x3 matrix."""
    c = np.array([[H[1, 1] * H[2, 2] - H[1, 2] * H[2, 1], H[0, 2] * H[2, 1] - H[0, 1] * H[2, 2],
                   H[0, 1] * H[1, 2] - H[0, 2] * H[1, 1]],
                  [H[1, 2] * H[2, 0] - H[1, 0] * H[2, 2], H[0, 0] * H[2, 2] - H[0, 2] * H[2, 0],
                   H[0, 2] * H[1, 0] - H[0, 0] * H[1, 2]],
                  [H[1, 0] * H[2, 1] - H[1, 1] * H[2, 0], H[0, 1] * H[2, 0] - H[0, 0] * H[2, 1],
                   H[0, 0] * H[1, 1] - H[0, 1] * H[1, 0]]])
    det = H[0, 0] * c[0, 0] + H[0, 1] * c[1, 0] + H[0, 2] * c[2, 0]
    return c / det


def _tri_solve(L, b, lower):
    try:
        from scipy.linalg import solve_triangular
        return solve_triangular(L, b, lower=lower)
    except ImportError:
        return np.linalg.solve(L, b)


class SysSBA:
    """SysSBA restricted to what sba_add uses: monocular projections, nFixed = 1, CHOLMOD solve, no Huber."""

    def __init__(self, camera=REFERENCE_SBA_CAMERA):
        self.camera = tuple(float(c) for c in camera)
        self.trans = []            # camera centres (3,)
        self.qrot = []             # (w, x, y, z)
        self.points = []           # (3,)
        self.tracks = []           # per point: {node index: (u, v)}
        self.lam = 1e-4            # doSBA's default (sba.h:158); sba_add always passes it
        self.log = []              # per iteration: cost before, cost after, lambda after, accepted, |x|^2

    # --- building (addNode / addPoint / addMonoProj) ---------------------------------------------------
    def add_node(self, pose7):
        p = np.asarray(pose7, dtype=np.float64)
        self.trans.append(p[:3].copy())
        self.qrot.append(norm_rot(p[3:7]))
        return len(self.trans) - 1

    def add_point(self, xyz):
        self.points.append(np.asarray(xyz, dtype=np.float64)[:3].copy())
        self.tracks.append({})
        return len(self.points) - 1

    def add_proj(self, ni, pi, uv):
        """addMonoProj: a repeat with the same keypoint is a no-op (True), a different one is rejected (False)."""
        kp = np.asarray(uv, dtype=np.float64)
        tr = self.tracks[pi]
        if ni in tr:
            return bool(np.array_equal(tr[ni], kp))
        tr[ni] = kp
        return True

    @property
    def nprojs(self):
        return sum(len(t) for t in self.tracks)

    # --- costs --------------------------------------------------------------------------------------------
    def _mats(self):
        return [node_mats(self.trans[i], self.qrot[i], self.camera) for i in range(len(self.trans))]

    def errors(self):
        """Squared error per projection, points ascending, nodes ascending within a point."""
        m = self._mats()
        out = []
        for pi, tr in enumerate(self.tracks):
            for ni in sorted(tr):
                out.append(proj_error(m[ni][1], self.points[pi], tr[ni])[1])
        return np.array(out, dtype=np.float64)

    def calc_cost(self):
        c = 0.0
        for e in self.errors():
            c += e
        return c

    def calc_rms_cost(self, dist=10000.0):
        d2 = dist * dist
        c, n = 0.0, 0
        for e in self.errors():
            if e < d2:
                c += e
                n += 1
        return math.sqrt(c / n) if n else float("nan")

    # --- one linear system -------------------------------------------------------------------------------
    def setup_sparse_sys(self, lam_in):
        """setupSparseSys + the diagonal scaling of setupCSstructure.  Returns (A dense, B, tps, Tpc)."""
        nn = len(self.trans)
        nfree = max(nn - 1, 0)
        m = self._mats()
        lam = 1.0 + lam_in
        A = np.zeros((6 * nfree, 6 * nfree))           # upper blocks as the reference stores them, mirrored below
        B = np.zeros(6 * nfree)
        tps = [np.zeros(3) for _ in self.points]
        Tpc = {}
        for pi, tr in enumerate(self.tracks):
            if not tr:
                continue
            X = self.points[pi]
            Hpp = np.zeros((3, 3))
            bp = np.zeros(3)
            jp = {}
            for ni in sorted(tr):
                w2n, w2i, dR = m[ni]
                e, _ = proj_error(w2i, X, tr[ni])
                jacc, jacp = proj_jacobians(w2n, dR, self.trans[ni], X, self.camera)
                jp[ni] = dict(Hpp=jacp.T @ jacp, Hcc=jacc.T @ jacc, Hpc=jacp.T @ jacc, JcTE=jacc.T @ e, Bp=jacp.T @ e)
                Hpp = Hpp + jp[ni]["Hpp"]
                bp = bp - jp[ni]["Bp"]
                if ni >= 1:
                    c = 6 * (ni - 1)
                    A[c:c + 6, c:c + 6] += jp[ni]["Hcc"]
                    B[c:c + 6] -= jp[ni]["JcTE"]
            Hpp[np.diag_indices(3)] *= lam
            Hppi = inv3(Hpp)
            tp = Hppi @ bp
            tps[pi] = tp
            free = [ni for ni in sorted(tr) if ni >= 1]
            for k, ni in enumerate(free):
                c = 6 * (ni - 1)
                B[c:c + 6] -= jp[ni]["Hpc"].T @ tp
                T = jp[ni]["Hpc"].T @ Hppi
                Tpc[(pi, ni)] = T
                for ni2 in free[k:]:
                    c2 = 6 * (ni2 - 1)
                    A[c:c + 6, c2:c2 + 6] += -(T @ jp[ni2]["Hpc"])
        iu = np.triu_indices(6 * nfree, 1)
        A.T[iu] = A[iu]                                  # the reference keeps the upper triangle
        A[np.diag_indices(6 * nfree)] *= lam
        # deviation 1: a free node without any projection gets an identity block and a zero right-hand side
        seen = set()
        for tr in self.tracks:
            seen.update(tr)
        for ni in range(1, nn):
            if ni not in seen:
                c = 6 * (ni - 1)
                A[c:c + 6, c:c + 6] = np.eye(6)
                B[c:c + 6] = 0.0
        return A, B, tps, Tpc

    @staticmethod
    def solve(A, B):
        """doChol: Cholesky, x = A^-1 B, one step of iterative refinement x += A^-1 (B - A x)."""
        try:
            L = np.linalg.cholesky(A)
        except np.linalg.LinAlgError as exc:
            raise NotPositiveDefinite(str(exc)) from None

        def chol_solve(b):
            y = _tri_solve(L, b, lower=True)
            return _tri_solve(L.T, y, lower=False)

        x = chol_solve(B)
        return x + chol_solve(B - A @ x)

    # --- the LM loop -------------------------------------------------------------------------------------
    def do_sba(self, niter, s_lambda=-1.0):
        """doSBA: returns the iteration count, -1 for an empty problem."""
        self.log = []
        nprjs = self.nprojs
        if nprjs == 0 or not self.points or not self.trans:
            return -1
        if s_lambda > 0.0:
            self.lam = s_lambda
        laminc, lamdec = 2.0, 0.5
        cost = self.calc_cost()
        it = 0
        while it < niter:
            A, B, tps, Tpc = self.setup_sparse_sys(self.lam)
            x = self.solve(A, B) if B.size else B
            sq = float(x @ x)
            if sq < SQ_MIN_DELTA:
                break
            old_t = [t.copy() for t in self.trans]
            old_q = [q.copy() for q in self.qrot]
            old_p = [p.copy() for p in self.points]
            for ni in range(1, len(self.trans)):
                c = 6 * (ni - 1)
                self.trans[ni] = self.trans[ni] + x[c:c + 3]
                v = x[c + 3:c + 6]
                qr = np.array([math.sqrt(1.0 - float(v @ v)), v[0], v[1], v[2]])
                q = quat_mul(self.qrot[ni], qr)
                self.qrot[ni] = q / math.sqrt(float(q @ q))
            for pi, tr in enumerate(self.tracks):
                if not tr:
                    continue
                tp = tps[pi].copy()
                for ni in sorted(tr):
                    if ni >= 1:
                        c = 6 * (ni - 1)
                        tp = tp - Tpc[(pi, ni)].T @ x[c:c + 6]
                self.points[pi] = self.points[pi] + tp
            newcost = self.calc_cost()
            before = cost
            if newcost < cost:
                cost = newcost
                self.lam *= lamdec
                acc = 1
            else:
                self.lam *= laminc
                laminc *= 2.0
                self.trans, self.qrot, self.points = old_t, old_q, old_p
                cost = self.calc_cost()
                acc = 0
            self.log.append((before, newcost, self.lam, acc, sq))
            it += 1
        return it

    def rms_wrapper(self):
        """SBANode::doSBA (sba_add.cpp:259-290)."""
        if not self.trans:
            return
        self.do_sba(10, 1e-4)
        c = self.calc_rms_cost()
        if math.isnan(c) or math.isinf(c):
            return
        if self.calc_rms_cost() > 4.0:
            self.do_sba(10, 1e-4)
        if self.calc_rms_cost() > 4.0:
            self.do_sba(15, 1e-4)

    def pose7(self):
        return np.array([np.concatenate([t, q]) for t, q in zip(self.trans, self.qrot)]).reshape(-1, 7)


def solve_refined(A, B, max_steps=20):
    """Test-only: the linear solve to numpy.longdouble accuracy.  The float64 Cholesky factor is the preconditioner of
    an iterative refinement whose residual and solution are kept in longdouble, until the correction stops shrinking.
    Against `SysSBA.solve` this measures how far float64 rounding in the solve alone moves the LM trajectory."""
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError as exc:
        raise NotPositiveDefinite(str(exc)) from None
    T = np.longdouble
    b = B.astype(T)

    def resid(x):
        out = np.empty(len(b), dtype=T)
        for r0 in range(0, len(b), 512):                 # row chunks: a 6138 x 6138 longdouble copy would be 600 MB
            out[r0:r0 + 512] = b[r0:r0 + 512] - A[r0:r0 + 512].astype(T) @ x
        return out

    x = np.zeros(len(b), dtype=T)
    last = np.inf
    for _ in range(max_steps):
        r = resid(x).astype(np.float64)
        dx = _tri_solve(L.T, _tri_solve(L, r, lower=True), lower=False)
        step = float(np.abs(dx).max()) if dx.size else 0.0
        if not step < last:
            break
        x = x + dx.astype(T)
        last = step
    return x.astype(np.float64)


class RefinedSolve:
    """Mix-in in front of SysSBA / RobustSysSBA: `solve` is `solve_refined` (test-only, see there)."""

    solve = staticmethod(solve_refined)


def sba_add(points_table, records, camera=REFERENCE_SBA_CAMERA, every=10, run=True):
    """The driver (SBANode::addFrame, sba_add.cpp:71-185) with deviation 3: points.txt row 0 is an ordinary point,
    `0 0 0` means no projection, P0 is a node id.  `points_table` is the N x 12 float32 table, `records` the
    (id, pose7 float32, projections) list of formats.read_pose_records.  Returns (sys, point rows, node ids); run=False
    only builds the problem."""
    s = SysSBA(camera)
    pts = np.asarray(points_table, dtype=np.float32)
    row_of = {}
    rows = []
    for i in range(pts.shape[0]):
        if pts[i, 0] or pts[i, 1] or pts[i, 2]:         # sba_add.cpp:106-108: zero rows are not added
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
        if run and every and len(s.trans) % every == 0:
            s.rms_wrapper()
    if run:
        s.rms_wrapper()
    return s, rows, ids
