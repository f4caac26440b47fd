"""Synthetic bundle-adjustment problems with gross outliers, for the robust SBA tests.

The conventions are those of `sba_scene.make_scene` (the trajectory, the pinhole camera, the cloud in front of node 0,
two points behind every camera, one projection-less free node, the perturbed start), with two differences that the
robust cost needs to show anything: every point is seen by 4 to 6 consecutive nodes (fewer only when the scene has
fewer), so that one wrong keypoint in a track is out-voted, and a stated share of the keypoints of points in front of
their camera is replaced by gross outliers, `outlier_px[0]` to `outlier_px[1]` pixels away in a random direction.
`scene["outlier"]` marks them.  There are no repeated projections here.
"""
from __future__ import annotations

import numpy as np

import sba_scene as sc

synthetic = sc.synthetic
CAMERA = sc.CAMERA


def make_robust_scene(n_free, n_points, seed=0, noise_px=0.5, outlier_share=0.05, outlier_px=(30.0, 80.0), dt=0.37,
                      lonely_node=True):
    rng = np.random.default_rng(seed)
    n_nodes = n_free + 1
    n_seen = n_nodes - 1 if (lonely_node and n_free >= 2) else n_nodes
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
    node, point, uv, front = [], [], [], []
    for j in range(n_points):
        k = min(int(rng.integers(4, 7)), n_seen)
        h = int(rng.integers(0, n_seen - k + 1))
        for i in range(h, h + k):
            c = Rs[i].T @ (pts[j] - poses[i, :3])
            if c[2] > 0:
                m = np.array([fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy]) + rng.normal(0, noise_px, 2)
            else:
                m = np.array([cx, cy])
            node.append(i)
            point.append(j)
            uv.append(m)
            front.append(c[2] > 0)
    node, point, uv = np.array(node, np.int32), np.array(point, np.int32), np.array(uv)
    outlier = np.zeros(len(node), bool)
    cand = np.flatnonzero(front)
    n_out = int(round(outlier_share * len(node)))
    pick = rng.choice(cand, n_out, replace=False)
    ang = rng.uniform(0, 2 * np.pi, n_out)
    mag = rng.uniform(outlier_px[0], outlier_px[1], n_out)
    uv[pick] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], axis=1)
    outlier[pick] = True
    start_nodes = poses.copy()
    for i in range(1, n_nodes):
        start_nodes[i, :3] += rng.normal(0, 0.01, 3)
        dq = np.concatenate([[1.0], rng.normal(0, 0.002, 3)])
        q = synthetic.quat_mul(poses[i, 3:], dq)
        start_nodes[i, 3:] = q / np.linalg.norm(q)
    start_points = pts + rng.normal(0, 0.02, pts.shape)
    return dict(camera=CAMERA, true_nodes=poses, true_points=pts, nodes=start_nodes, points=start_points,
                node=node, point=point, uv=uv, outlier=outlier, scale=float(np.abs(pts).max()))


def oracle_system(scene, huber=0.0, keep=None):
    """The robust oracle over the scene; `keep` (bool per projection) adds only those, in the scene's order."""
    import sba_robust_oracle as ro
    s = ro.RobustSysSBA(scene["camera"], huber)
    for p in scene["nodes"]:
        s.add_node(p)
    for x in scene["points"]:
        s.add_point(x)
    for k, (ni, pi, m) in enumerate(zip(scene["node"], scene["point"], scene["uv"])):
        if keep is None or keep[k]:
            s.add_proj(int(ni), int(pi), m)
    return s


def pose_error(nodes, scene):
    """RMS distance of the camera centres of the nodes with projections from `true_nodes` (world units)."""
    seen = np.unique(scene["node"])
    d = np.asarray(nodes)[seen, :3] - scene["true_nodes"][seen, :3]
    return float(np.sqrt((d * d).sum(axis=1).mean()))
