"""Synthetic bundle-adjustment problems whose reduced camera system is not a narrow band.

`sba_scene.make_scene` and `sba_robust_scene.make_robust_scene` give every point to a few consecutive nodes, so their
camera systems are block-banded with a half-bandwidth of at most 5 blocks.  The scenes here keep their conventions (the
camera, `synthetic.trajectory`, the cloud in front of node 0, two points behind every camera, five repeated
projections, one projection-less free node, the perturbed start, the same dict keys) and differ in which nodes see a
point:

- `dense`:   about 30 % of the points get a track length uniform in [2, max_track], the others 2-3 (`min_track` raises
             both lower ends); the nodes of a track are drawn without replacement from the whole trajectory.  Every
             pair of seen free nodes shares points: a full matrix, long tracks, long pair item lists.
- `loop`:    consecutive tracks of 2-3 nodes, plus points seen by two of the first four and two of the last four seen
             nodes: a band and a far corner block, whose fill-in spreads through the whole trailing matrix.
- `hub`:     consecutive tracks of 2-3 nodes, plus one free node in the middle that sees about 90 % of the points: an
             arrow matrix, one neighbour list of nearly every other node.
- `islands`: the seen free nodes fall into two groups; a point belongs to one group and is seen by 2-8 of its nodes,
             drawn from anywhere in the group, and by node 0 with probability 0.3.  The blocks between the two groups
             are absent.  `quiet_second` leaves the second island at the truth (nodes and points unperturbed, no
             keypoint noise, no rejected repeat, keypoints through the attitude as the solver normalises it): its
             right-hand side is rounding only.

`outlier_share` (dense) replaces that share of the keypoints by 30-80 px outliers, as `make_robust_scene`, and
`doomed_pairs` picks that many far pairs of free nodes (|a - b| > 42, or the farthest third below that size) and makes
every point they share an outlier at the pair's lower node: once these are pruned the pair's block is gone.

`structure(scene)` computes the facts the tests rely on from scene["node"] and scene["point"] alone.
"""
from __future__ import annotations

import numpy as np

import sba_scene as sc

synthetic = sc.synthetic
CAMERA = sc.CAMERA
KINDS = ("dense", "loop", "hub", "islands")


def _consecutive(rng, n_seen):
    k = 2 if (n_seen <= 2 or rng.random() < 0.5) else 3
    h = int(rng.integers(0, n_seen - k + 1)) if n_seen > k else 0
    return list(range(h, min(h + k, n_seen)))


def island_groups(n_free, lonely_node=True):
    """The free nodes (1-based node indices) of the two islands."""
    n_seen = n_free if (lonely_node and n_free >= 2) else n_free + 1
    half = (n_seen - 1) // 2
    return list(range(1, 1 + half)), list(range(1 + half, n_seen))


def _tracks(kind, rng, n_free, n_seen, n_points, max_track, min_track):
    tracks = []
    if kind == "dense":
        top = min(max_track, n_seen)
        for _ in range(n_points):
            if rng.random() < 0.3:
                k = int(rng.integers(min(min_track, top), top + 1))
            else:
                k = min(int(rng.integers(min_track, min_track + 2)), n_seen)
            tracks.append(sorted(int(i) for i in rng.choice(n_seen, k, replace=False)))
    elif kind == "loop":
        n_loop = max(8, n_points // 10)
        w = min(4, n_seen // 2)
        for j in range(n_points):
            if j % (n_points // n_loop) == 0 and w >= 2:
                head = rng.choice(w, 2, replace=False)
                tail = n_seen - 1 - rng.choice(w, 2, replace=False)
                tracks.append(sorted(int(i) for i in np.concatenate([head, tail])))
            else:
                tracks.append(_consecutive(rng, n_seen))
    elif kind == "hub":
        hub = n_seen // 2
        for _ in range(n_points):
            t = _consecutive(rng, n_seen)
            if rng.random() < 0.9 and hub not in t:
                t = sorted(t + [hub])
            tracks.append(t)
    elif kind == "islands":
        groups = island_groups(n_free, n_seen == n_free)
        for j in range(n_points):
            g = groups[j % 2]
            k = int(rng.integers(2, min(8, len(g)) + 1))
            t = [int(i) for i in rng.choice(g, k, replace=False)]
            if rng.random() < 0.3:
                t.append(0)
            tracks.append(sorted(t))
    else:
        raise ValueError("kind must be one of %s" % (KINDS,))
    return tracks


def make_topology_scene(kind, n_free, n_points, seed=0, noise_px=0.5, dt=0.37, lonely_node=True, max_track=60,
                        min_track=2, outlier_share=0.0, outlier_px=(30.0, 80.0), doomed_pairs=0, quiet_second=False):
    rng = np.random.default_rng(seed)
    n_nodes = n_free + 1
    n_seen = n_nodes - 1 if (lonely_node and n_free >= 2) else n_nodes      # the last node stays projection-less
    poses, Rs = [], []
    for i in range(n_nodes):
        r, q = synthetic.trajectory(i * dt)
        poses.append(np.concatenate([r, q]))
        Rs.append(synthetic.quat2rot(q))
    poses = np.array(poses)
    fx, fy, cx, cy = CAMERA
    n_behind = 2 if n_points >= 20 else 0
    n_front = n_points - n_behind
    pc = np.stack([rng.uniform(-0.4, 0.4, n_front), rng.uniform(-0.3, 0.3, n_front),
                   rng.uniform(*synthetic.DEPTH, n_front)], axis=1)
    pc[:, :2] *= pc[:, 2:3]
    pts = poses[0, :3] + pc @ Rs[0].T
    behind = poses[0, :3] + np.array([[0.2, 0.1, -3.0], [-0.3, 0.0, -4.0]])[:n_behind] @ Rs[0].T
    pts = np.vstack([pts, behind])
    tracks = _tracks(kind, rng, n_free, n_seen, n_points, max_track, min_track)
    second = set(island_groups(n_free, lonely_node)[1]) if kind == "islands" else set()
    quiet_pt = np.array([quiet_second and bool(second.intersection(t)) for t in tracks])
    # The solver normalises every attitude on add (Node::normRot), which turns the trajectory's half-turn attitudes by
    # about 0.03 rad; the quiet island's keypoints are projected through that attitude, so that its errors are rounding.
    if quiet_second:
        import sba_oracle as so
        Rn = [so.quat_rot(so.norm_rot(p[3:])) for p in poses]
    node, point, uv, front = [], [], [], []
    for j, t in enumerate(tracks):
        for i in t:
            c = (Rn[i] if quiet_pt[j] else Rs[i]).T @ (pts[j] - poses[i, :3])
            if c[2] > 0:
                m = np.array([fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy])
                noise = rng.normal(0, noise_px, 2)
                if not quiet_pt[j]:
                    m = m + noise
            else:
                m = np.array([cx, cy])
            node.append(i)
            point.append(j)
            uv.append(m)
            front.append(c[2] > 0)
    node, point, uv = np.array(node, np.int32), np.array(point, np.int32), np.array(uv)
    front = np.array(front)
    outlier = np.zeros(len(node), bool)
    doomed = []
    if doomed_pairs:
        far = min(42, (2 * n_free) // 3)
        seen_by = [set(point[node == i].tolist()) for i in range(n_nodes)]
        while len(doomed) < doomed_pairs:
            a, b = sorted(int(i) for i in rng.choice(np.arange(1, n_seen), 2, replace=False))
            shared = seen_by[a] & seen_by[b]
            if b - a <= far or not shared or (a, b) in doomed:
                continue
            doomed.append((a, b))
            outlier |= (node == a) & np.isin(point, list(shared)) & front
    if outlier_share > 0.0:
        cand = np.flatnonzero(front & ~outlier)
        outlier[rng.choice(cand, int(round(outlier_share * len(node))), replace=False)] = True
    n_out = int(outlier.sum())
    if n_out:
        ang = rng.uniform(0, 2 * np.pi, n_out)
        mag = rng.uniform(outlier_px[0], outlier_px[1], n_out)
        uv[outlier] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
    # repeats: three exact (no-ops), two with another keypoint (rejected)
    dup = rng.choice(np.flatnonzero(~quiet_pt[point]) if quiet_second else len(node), 5, replace=False)
    d_uv = uv[dup].copy()
    d_uv[3:] += 7.0
    node = np.concatenate([node, node[dup]])
    point = np.concatenate([point, point[dup]])
    uv = np.concatenate([uv, d_uv])
    outlier = np.concatenate([outlier, np.zeros(5, bool)])
    start_nodes = poses.copy()
    for i in range(1, n_nodes):
        dr = rng.normal(0, 0.01, 3)
        dq = np.concatenate([[1.0], rng.normal(0, 0.002, 3)])
        if quiet_second and i in second:
            continue
        start_nodes[i, :3] += dr
        q = synthetic.quat_mul(poses[i, 3:], dq)
        start_nodes[i, 3:] = q / np.linalg.norm(q)
    start_points = pts + rng.normal(0, 0.02, pts.shape) * (~quiet_pt)[:, None]
    return dict(camera=CAMERA, true_nodes=poses, true_points=pts, nodes=start_nodes, points=start_points,
                node=node, point=point, uv=uv, outlier=outlier, doomed=doomed, kind=kind,
                scale=float(np.abs(pts).max()))


def pair_set(node, point, valid=None):
    """The off-diagonal pairs (a, b), a < b, of 0-based free-node indices that share at least one point."""
    node, point = np.asarray(node), np.asarray(point)
    if valid is not None:
        node, point = node[valid], point[valid]
    by_point = {}
    for n, p in zip(node.tolist(), point.tolist()):
        if n >= 1:
            by_point.setdefault(p, set()).add(n - 1)
    pairs = set()
    for s in by_point.values():
        s = sorted(s)
        pairs.update((a, b) for k, a in enumerate(s) for b in s[k + 1:])
    return pairs


def structure(scene):
    """Facts about the reduced camera system, from scene["node"] and scene["point"] alone."""
    node, point = scene["node"], scene["point"]
    n_free = len(scene["nodes"]) - 1
    pairs = pair_set(node, point)
    seen_free = sorted({int(n) - 1 for n in node if n >= 1})
    deg = np.zeros(max(n_free, 1), int)
    for a, b in pairs:
        deg[a] += 1
        deg[b] += 1
    track = {}
    for n, p in set(zip(node.tolist(), point.tolist())):
        track[p] = track.get(p, 0) + 1
    ns = len(seen_free)
    return dict(pairs=pairs, n_pairs=len(pairs), seen_free=seen_free,
                pair_fraction=len(pairs) / max(ns * (ns - 1) // 2, 1),
                max_span=max((b - a for a, b in pairs), default=0),
                longest_track=max(track.values()), max_degree=int(deg.max()), degree=deg)


# --- the scenes the topology tests use (tests/golden/sba_topology_bounds.json holds what was measured on them) -------
# (kind, free nodes, points, seed)
NITER = 5                                         # LM iterations of a full run: see tests/test_oracle_sba_topology.py
CHOL_CASES = [("dense", 10, 120, 0), ("dense", 11, 120, 0), ("dense", 32, 300, 0), ("dense", 59, 300, 0),
              ("dense", 127, 600, 2), ("loop", 59, 300, 0), ("loop", 127, 600, 0), ("hub", 59, 300, 0),
              ("hub", 127, 600, 0), ("islands", 59, 300, 0), ("islands", 127, 600, 0)]
PCG_CASES = [(k, f, 10 * f, 0) for k in ("dense", "hub", "loop") for f in (41, 42, 43)] + \
            [("dense", 127, 600, 2), ("hub", 127, 600, 0), ("loop", 127, 600, 0)]
PCG_TIGHT = (1e-30, 4000)                         # a CG that converges on every scene above (asserted on the CPU)
CAP_CASE = ("loop", 1023, 3000, 0)                # the Cholesky handle's largest system: n6 = 6138, npad = 6144
BITWISE_CASE = ("dense", 127, 600, 2)
ROBUST_CASE = dict(kind="dense", n_free=59, n_points=300, seed=0, max_track=12, min_track=4, outlier_share=0.03,
                   doomed_pairs=6)
ONE_STEP_CASES = [("dense", 59, 300, 0), ("islands", 59, 300, 0)]
# Scenes whose own float64-vs-longdouble spread, times 10, exceeds the project bound (STATE_TOL for a Cholesky handle,
# 1e-9 for a converged CG): their bound is 10 x that spread (tests/golden/sba_topology_bounds.json).
OWN_BOUND = set()


def case_scene(kind, nfree, npts, seed, **kw):
    return make_topology_scene(kind, nfree, npts, seed=seed, **kw)


# --- oracles over a scene, in float64 and with the linear solve in longdouble ----------------------------------------
def _fill(s, scene, keep=None):
    for p in scene["nodes"]:
        s.add_node(p)
    for x in scene["points"]:
        s.add_point(x)
    for k, (ni, pi, m) in enumerate(zip(scene["node"], scene["point"], scene["uv"])):
        if keep is None or keep[k]:
            s.add_proj(int(ni), int(pi), m)
    return s


def cholesky_oracle(scene, huber=None, longdouble=False):
    """sba_oracle.SysSBA (RobustSysSBA with `huber`); `longdouble` swaps its solve for sba_oracle.solve_refined."""
    import sba_oracle as so
    import sba_robust_oracle as ro
    base = so.SysSBA if huber is None else ro.RobustSysSBA
    cls = type("Refined" + base.__name__, (so.RefinedSolve, base), {}) if longdouble else base
    return _fill(cls(scene["camera"]) if huber is None else cls(scene["camera"], huber), scene)


def pcg_oracle(scene, cg, huber=None, longdouble=False):
    """sba_pcg_oracle's system with the CG settings `cg` = (tol, max_iters), its arithmetic float64 or longdouble."""
    import sba_pcg_oracle as po
    return po.pcg_system(scene, huber).set_cg(*cg, dtype=np.longdouble if longdouble else np.float64)


def state_spread(a, b):
    """max |difference| of the nodes and points of two oracles."""
    return max(float(np.abs(a.pose7() - b.pose7()).max()),
               float(np.abs(np.array(a.points) - np.array(b.points)).max()))


def tie_margin(ref):
    """min over the logged iterations of |newcost - cost| / cost: how far every accept / reject decision is from a tie."""
    log = np.array(ref.log, dtype=np.float64).reshape(-1, 5)
    return float(np.min(np.abs(log[:, 1] - log[:, 0]) / log[:, 0])) if len(log) else float("inf")
