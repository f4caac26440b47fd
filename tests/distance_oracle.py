"""The mesh-to-mesh distance of DESIGN.md §31 restated in numpy, twice: ``distance_loop`` walks points and triangles with Python
floats, ``distance`` is vectorised over both; ``grid_walk`` is a model of the device's grid search and its termination rule, and
``stats`` of the fixed-order statistics.  The contract (include/ekf_monoslam.h, csrc/ekf_mesh_distance.hpp), fp64, every operation
rounded once, in the written order:

  1. a triangle (i0, i1, i2) with the corners A, B, C is valid iff its indices are distinct, its nine coordinates are finite and,
     with u = B - A, v = C - A, n = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0), nn = (n0 n0 + n1 n1) + n2 n2 is finite and > 0;
  2. Ericson's closest point (Real-Time Collision Detection, §5.1.5), dot(a, b) = (a0 b0 + a1 b1) + a2 b2:
       d1 = dot(ab, ap), d2 = dot(ac, ap);  d1 <= 0 and d2 <= 0:                                  c = A
       d3 = dot(ab, bp), d4 = dot(ac, bp);  d3 >= 0 and d4 <= d3:                                 c = B
       vc = d1 d4 - d3 d2;  vc <= 0 and d1 >= 0 and d3 <= 0:      v = d1 / (d1 - d3),             c = A + v ab
       d5 = dot(ab, cp), d6 = dot(ac, cp);  d6 >= 0 and d5 <= d6:                                 c = C
       vb = d5 d2 - d1 d6;  vb <= 0 and d2 >= 0 and d6 <= 0:      w = d2 / (d2 - d6),             c = A + w ac
       va = d3 d6 - d5 d4, e = d4 - d3, f = d5 - d6;  va <= 0 and e >= 0 and f >= 0:  w = e / (e + f),  c = B + w (C - B)
       otherwise s = (va + vb) + vc, v = vb / s, w = vc / s,                                      c = (A + v ab) + w ac
     then c is clamped to the triangle's own box by comparisons (a NaN stays), q = p - c, d2 = (q0 q0 + q1 q1) + q2 q2;
  3. the least (d2, t) over the valid triangles: t replaces the best iff d2 < best or d2 == best and t < best_t, from
     (+inf, 0xffffffff); dist = sqrt(d2), tri, closest, side = sign((q0 n0 + q1 n1) + q2 n2); a point that is not finite gets
     NaN, 0xffffffff, NaN, 0;
  5. statistics: see ``stats``.
"""
import math

import numpy as np

NO_TRI = 0xFFFFFFFF
HUGE = 1.7976931348623157e308
SLACK = 2.0 ** -40
MAG_LO, MAG_HI = 2.0 ** -400, 2.0 ** 400
MAX_G = 128


def _mesh(mesh):
    X = np.ascontiguousarray(mesh["vertices"], np.float64).reshape(-1, 3)
    F = np.ascontiguousarray(mesh["faces"]).reshape(-1, 3).astype(np.int64)
    return X, F


# ---- the loop form -------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _div(a, b):
    """a / b of IEEE doubles: Python raises on a zero divisor."""
    if b == 0.0:
        if a != a or a == 0.0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def normal_loop(A, B, C):
    u, v = _sub(B, A), _sub(C, A)
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def valid_loop(idx, A, B, C):
    if idx[0] == idx[1] or idx[1] == idx[2] or idx[0] == idx[2]:
        return False
    if not all(abs(x) <= HUGE for x in tuple(A) + tuple(B) + tuple(C)):
        return False
    n = normal_loop(A, B, C)
    nn = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]
    return nn > 0.0 and nn <= HUGE


def closest_loop(p, A, B, C):
    """(d2, c) of step 2."""
    ab, ac, ap = _sub(B, A), _sub(C, A), _sub(p, A)
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = _sub(p, B)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = _sub(p, C)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    e, f = d4 - d3, d5 - d6
    if d1 <= 0.0 and d2 <= 0.0:
        c = tuple(A)
    elif d3 >= 0.0 and d4 <= d3:
        c = tuple(B)
    elif vc <= 0.0 and d1 >= 0.0 and d3 <= 0.0:
        v = _div(d1, d1 - d3)
        c = tuple(A[k] + v * ab[k] for k in range(3))
    elif d6 >= 0.0 and d5 <= d6:
        c = tuple(C)
    elif vb <= 0.0 and d2 >= 0.0 and d6 <= 0.0:
        w = _div(d2, d2 - d6)
        c = tuple(A[k] + w * ac[k] for k in range(3))
    elif va <= 0.0 and e >= 0.0 and f >= 0.0:
        w = _div(e, e + f)
        c = tuple(B[k] + w * (C[k] - B[k]) for k in range(3))
    else:
        s = (va + vb) + vc
        v, w = _div(vb, s), _div(vc, s)
        c = tuple((A[k] + v * ab[k]) + w * ac[k] for k in range(3))
    out = []
    for k in range(3):
        lo = hi = A[k]
        if B[k] < lo:
            lo = B[k]
        if C[k] < lo:
            lo = C[k]
        if B[k] > hi:
            hi = B[k]
        if C[k] > hi:
            hi = C[k]
        out.append(lo if c[k] < lo else (hi if c[k] > hi else c[k]))
    q = _sub(p, out)
    return (q[0] * q[0] + q[1] * q[1]) + q[2] * q[2], tuple(out)


def _empty(n):
    return dict(dist=np.full(n, np.nan), tri=np.full(n, NO_TRI, np.uint32), closest=np.full((n, 3), np.nan), side=np.zeros(n, np.int8),
                d2=np.full(n, np.nan))


def distance_loop(mesh, points):
    """dist, tri, closest, side (and d2) of every point, one triangle at a time; None if no triangle is valid."""
    X, F = _mesh(mesh)
    P = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    tris = [(t, tuple(map(float, X[i])), tuple(map(float, X[j])), tuple(map(float, X[k]))) for t, (i, j, k) in enumerate(F.tolist())
            if valid_loop((i, j, k), X[i], X[j], X[k])]
    if not tris:
        return None
    out = _empty(len(P))
    for i, p in enumerate(P.tolist()):
        if not all(abs(x) <= HUGE for x in p):
            continue
        best, bt, bc = math.inf, NO_TRI, None
        for t, A, B, C in tris:
            d2, c = closest_loop(p, A, B, C)
            if d2 < best or (d2 == best and t < bt):
                best, bt, bc = d2, t, (c, A, B, C)
        if bt == NO_TRI:
            continue
        c, A, B, C = bc
        n, q = normal_loop(A, B, C), _sub(p, c)
        s = _dot(q, n)
        out["d2"][i], out["dist"][i], out["tri"][i], out["closest"][i] = best, math.sqrt(best), bt, c
        out["side"][i] = 1 if s > 0.0 else (-1 if s < 0.0 else 0)
    return out


# ---- the vectorised form ---------------------------------------------------------------------------------------------------------
def _vdot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def normals(X, F):
    A, B, C = X[F[:, 0]], X[F[:, 1]], X[F[:, 2]]
    u, v = B - A, C - A
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], axis=1)


def valid(X, F):
    with np.errstate(all="ignore"):
        A, B, C = X[F[:, 0]], X[F[:, 1]], X[F[:, 2]]
        distinct = (F[:, 0] != F[:, 1]) & (F[:, 1] != F[:, 2]) & (F[:, 0] != F[:, 2])
        finite = (np.abs(np.concatenate([A, B, C], axis=1)) <= HUGE).all(axis=1)
        n = normals(X, F)
        nn = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
        return distinct & finite & (nn > 0.0) & (nn <= HUGE)


def closest(P, A, B, C):
    """Step 2 for points P (n, 3) against triangles A, B, C (m, 3): d2 (n, m) and c (3, n, m)."""
    with np.errstate(all="ignore"):
        p = [P[:, k][:, None] for k in range(3)]
        a, b, c = ([T[:, k][None, :] for k in range(3)] for T in (A, B, C))
        ab, ac = [b[k] - a[k] for k in range(3)], [c[k] - a[k] for k in range(3)]
        ap, bp, cp = ([p[k] - t[k] for k in range(3)] for t in (a, b, c))
        d1, d2 = _vdot(ab, ap), _vdot(ac, ap)
        d3, d4 = _vdot(ab, bp), _vdot(ac, bp)
        d5, d6 = _vdot(ab, cp), _vdot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e, f = d4 - d3, d5 - d6
        rA = (d1 <= 0.0) & (d2 <= 0.0)
        rB = (d3 >= 0.0) & (d4 <= d3)
        rAB = (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0)
        rC = (d6 >= 0.0) & (d5 <= d6)
        rAC = (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0)
        rBC = (va <= 0.0) & (e >= 0.0) & (f >= 0.0)
        v_ab = d1 / (d1 - d3)
        w_ac = d2 / (d2 - d6)
        w_bc = e / (e + f)
        s = (va + vb) + vc
        v_in, w_in = vb / s, vc / s
        out = []
        for k in range(3):
            q = (a[k] + v_in * ab[k]) + w_in * ac[k]
            q = np.where(rBC, b[k] + w_bc * (c[k] - b[k]), q)
            q = np.where(rAC, a[k] + w_ac * ac[k], q)
            q = np.where(rC, np.broadcast_to(c[k], q.shape), q)
            q = np.where(rAB, a[k] + v_ab * ab[k], q)
            q = np.where(rB, np.broadcast_to(b[k], q.shape), q)
            q = np.where(rA, np.broadcast_to(a[k], q.shape), q)
            lo = np.where(b[k] < a[k], b[k], a[k])
            lo = np.where(c[k] < lo, c[k], lo)
            hi = np.where(b[k] > a[k], b[k], a[k])
            hi = np.where(c[k] > hi, c[k], hi)
            out.append(np.where(q < lo, lo, np.where(q > hi, hi, q)))
        r = [p[k] - out[k] for k in range(3)]
        return (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2], out


def distance(mesh, points, chunk=256, want_d2=False):
    """The vectorised form: dist, tri, closest, side and d2 of every point; None if no triangle is valid.  ``want_d2`` also keeps
    the whole matrix of d2 (points x triangles, NaN for an invalid triangle), which ``grid_walk`` looks values up in."""
    X, F = _mesh(mesh)
    P = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    ok = valid(X, F)
    if not ok.any():
        return None
    ids = np.flatnonzero(ok)
    A, B, C = X[F[ids, 0]], X[F[ids, 1]], X[F[ids, 2]]
    N = normals(X, F[ids])
    out = _empty(len(P))
    if want_d2:
        out["matrix"] = np.full((len(P), len(F)), np.nan)
    good = (np.abs(P) <= HUGE).all(axis=1)
    with np.errstate(all="ignore"):
        for i0 in range(0, len(P), chunk):
            sel = np.flatnonzero(good[i0:i0 + chunk]) + i0
            if not len(sel):
                continue
            d2, c = closest(P[sel], A, B, C)
            if want_d2:
                out["matrix"][np.ix_(sel, ids)] = d2
            any_ = ~np.isnan(d2).all(axis=1)
            best = np.nanmin(np.where(any_[:, None], d2, 0.0), axis=1)
            j = np.argmax(d2 == best[:, None], axis=1)                        # the first: ids ascend, so the least index
            rows = np.arange(len(sel))
            cw = np.stack([c[k][rows, j] for k in range(3)], axis=1)
            q = P[sel] - cw
            s = (q[:, 0] * N[j, 0] + q[:, 1] * N[j, 1]) + q[:, 2] * N[j, 2]
            w = sel[any_]
            out["d2"][w] = best[any_]
            out["dist"][w] = np.sqrt(best[any_])
            out["tri"][w] = ids[j[any_]]
            out["closest"][w] = cw[any_]
            out["side"][w] = np.where(s > 0.0, 1, np.where(s < 0.0, -1, 0))[any_]
    return out


# ---- the statistics ---------------------------------------------------------------------------------------------------------------
def _tree(v):
    """v (..., 256): for s = 128 .. 1: v[l] += v[l + s]."""
    v = np.array(v, np.float64)
    s = 128
    while s:
        v[..., :s] = v[..., :s] + v[..., s:2 * s]
        s //= 2
    return v[..., 0]


def _fixed_sum(values):
    """Step 5's order: blocks of 256 by the tree; lane l adds the partials l, l + 256, .. in ascending order from 0.0; the tree."""
    n = len(values)
    nblk = (n + 255) // 256
    v = np.zeros(nblk * 256)
    v[:n] = values
    part = _tree(v.reshape(nblk, 256))
    rows = (nblk + 255) // 256
    p = np.zeros(rows * 256)
    p[:nblk] = part
    acc = np.zeros(256)
    for row in p.reshape(rows, 256):
        acc = acc + row
    return float(_tree(acc))


def stats(dist, thr):
    """n, n_bad, max, argmax, mean, rms, within, sum, sum2 of step 5."""
    d = np.asarray(dist, np.float64)
    bad = np.isnan(d)
    n, n_bad = int((~bad).sum()), int(bad.sum())
    z = np.where(bad, 0.0, d)
    total, total2 = _fixed_sum(z), _fixed_sum(z * z)
    if n == 0:
        return dict(n=0, n_bad=n_bad, max=math.nan, argmax=NO_TRI, mean=math.nan, rms=math.nan, within=0, sum=total, sum2=total2)
    arg = int(np.argmax(np.where(bad, -1.0, d)))
    with np.errstate(all="ignore"):
        return dict(n=n, n_bad=n_bad, max=float(d[arg]), argmax=arg, mean=total / n, rms=math.sqrt(total2 / n),
                    within=int((d[~bad] <= thr).sum()), sum=total, sum2=total2)


def stats_loop(dist, thr):
    """The same, one value at a time."""
    d = [float(x) for x in np.asarray(dist, np.float64)]

    def tree(v):
        v, s = list(v), 128
        while s:
            for l in range(s):
                v[l] = v[l] + v[l + s]
            s //= 2
        return v[0]

    def fixed(vals):
        vals = vals + [0.0] * (-len(vals) % 256)
        part = [tree(vals[b:b + 256]) for b in range(0, len(vals), 256)]
        acc = [0.0] * 256
        for lane in range(256):
            for b in range(lane, len(part), 256):
                acc[lane] = acc[lane] + part[b]
        return tree(acc)

    good = [x for x in d if x == x]
    n = len(good)
    total, total2 = fixed([x if x == x else 0.0 for x in d]), fixed([x * x if x == x else 0.0 for x in d])
    if n == 0:
        return dict(n=0, n_bad=len(d), max=math.nan, argmax=NO_TRI, mean=math.nan, rms=math.nan, within=0, sum=total, sum2=total2)
    mx = max(good)
    return dict(n=n, n_bad=len(d) - n, max=mx, argmax=d.index(mx), mean=total / n, rms=math.sqrt(total2 / n),
                within=sum(1 for x in good if x <= thr), sum=total, sum2=total2)


# ---- a model of the grid search ----------------------------------------------------------------------------------------------------
def auto_g(n_valid):
    return int(min(MAX_G, max(1, math.ceil(math.sqrt(n_valid / 2.0)))))


def make_grid(X, F, g=0):
    """The box of the valid triangles' vertices and the cells: lo, hi, h (3 floats each), G (3 ints), mag."""
    ok = valid(X, F)
    V = X[F[ok].reshape(-1)]
    lo, hi = [float(x) for x in V.min(axis=0)], [float(x) for x in V.max(axis=0)]
    g = g or auto_g(int(ok.sum()))
    mag = max(max(abs(a), abs(b)) for a, b in zip(lo, hi))
    longest = max(b - a for a, b in zip(lo, hi))
    if not (MAG_LO <= mag <= MAG_HI) or not longest > 0.0:
        g = 1
    G, h = [], []
    for a, b in zip(lo, hi):
        ext = b - a
        want = math.ceil(g * (ext / longest))
        G.append(g if want >= g else (int(want) if want > 1.0 else 1))
        h.append(ext / G[-1])
    return dict(lo=lo, hi=hi, h=h, G=G, mag=mag)


def cell(grid, k, x):
    q = _div(x - grid["lo"][k], grid["h"][k])
    top = grid["G"][k] - 1
    if q != q:
        return 0
    q = math.floor(q) if abs(q) != math.inf else q
    return top if q >= top else (int(q) if q > 0.0 else 0)


def file_triangles(X, F, grid):
    """cell (x, y, z) -> the triangles filed there, and the longest list."""
    cells = {}
    for t in np.flatnonzero(valid(X, F)):
        V = X[F[t]]
        r = [(cell(grid, k, float(V[:, k].min())), cell(grid, k, float(V[:, k].max()))) for k in range(3)]
        for z in range(r[2][0], r[2][1] + 1):
            for y in range(r[1][0], r[1][1] + 1):
                for x in range(r[0][0], r[0][1] + 1):
                    cells.setdefault((x, y, z), []).append(int(t))
    return cells


def grid_walk(mesh, points, g, matrix, strict=True, slack=SLACK):
    """The device's search, shell by shell, with d2 looked up in ``matrix`` (``distance(..., want_d2=True)``): the winning
    (d2, tri) of every point, the shells every point visited and the triangles it evaluated.  ``strict=False`` or ``slack=0``
    give the rules that the tie across shells exists to catch."""
    X, F = _mesh(mesh)
    P = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
    grid = make_grid(X, F, g)
    cells = file_triangles(X, F, grid)
    G, lo, hi, h = grid["G"], grid["lo"], grid["hi"], grid["h"]
    d2s, tris, shells, evals = np.full(len(P), np.nan), np.full(len(P), NO_TRI, np.uint32), np.zeros(len(P), int), np.zeros(len(P), int)
    for i, p in enumerate(P.tolist()):
        if not all(abs(x) <= HUGE for x in p):
            continue
        pc = [min(max(p[k], lo[k]), hi[k]) for k in range(3)]
        c = [cell(grid, k, pc[k]) for k in range(3)]
        mag = max(grid["mag"], abs(p[0]), abs(p[1]), abs(p[2]))
        sl = slack * mag
        best, bt, r = math.inf, NO_TRI, 0
        while True:
            for z in range(max(c[2] - r, 0), min(c[2] + r, G[2] - 1) + 1):
                for y in range(max(c[1] - r, 0), min(c[1] + r, G[1] - 1) + 1):
                    for x in range(max(c[0] - r, 0), min(c[0] + r, G[0] - 1) + 1):
                        if max(abs(x - c[0]), abs(y - c[1]), abs(z - c[2])) != r:
                            continue
                        for t in cells.get((x, y, z), ()):
                            d2 = matrix[i, t]
                            evals[i] += 1
                            if d2 < best or (d2 == best and t < bt):
                                best, bt = d2, t
            shells[i] = r + 1
            if all(c[k] - r <= 0 and c[k] + r >= G[k] - 1 for k in range(3)):
                break
            m = math.inf
            for k in range(3):
                if c[k] + r < G[k] - 1:
                    m = min(m, (lo[k] + float(c[k] + r + 1) * h[k]) - pc[k])
                if c[k] - r > 0:
                    m = min(m, pc[k] - (lo[k] + float(c[k] - r) * h[k]))
            lb = m - sl
            if mag <= MAG_HI and lb >= sl and (best < lb * lb if strict else best <= lb * lb):
                break
            r += 1
        if bt != NO_TRI:
            d2s[i], tris[i] = best, bt
    return dict(d2=d2s, tri=tris, shells=shells, evals=evals, grid=grid, longest=max(len(v) for v in cells.values()))
