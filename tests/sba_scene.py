"""Synthetic bundle-adjustment problems shared by the SBA tests.

Cameras follow `synthetic.trajectory` (attitude through `synthetic.quat2rot`) and look at a static cloud through a
pinhole K.  Every point is seen by two or three consecutive nodes; on top of that the scene holds
- two points behind every camera (their projections have p1.z <= 0: zero error, Hessian terms kept),
- repeated projections (same keypoint: a no-op; different keypoint: rejected),
- one free node without any projection (deviation 1),
and a perturbed start for nodes 1.. and every point.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ekf-monoslam_for_3d-reconstruction_amd"))
import synthetic  # noqa: E402

sys.path.pop(0)

CAMERA = (520.0, 520.0, 320.0, 240.0)


def make_scene(n_free, n_points, seed=0, noise_px=0.5, dt=0.37, lonely_node=True):
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
    # the cloud, in front of node 0 (camera frame: z along the optical axis)
    n_behind = 2 if n_points >= 20 else 0
    n_front = n_points - n_behind
    pc = np.stack([rng.uniform(-0.4, 0.4, n_front), rng.uniform(-0.3, 0.3, n_front),
                   rng.uniform(*synthetic.DEPTH, n_front)], axis=1)
    pc[:, :2] *= pc[:, 2:3]
    pts = poses[0, :3] + pc @ Rs[0].T
    behind = poses[0, :3] + np.array([[0.2, 0.1, -3.0], [-0.3, 0.0, -4.0]])[:n_behind] @ Rs[0].T
    pts = np.vstack([pts, behind])
    node, point, uv = [], [], []
    for j in range(n_points):
        k = 2 if (n_seen <= 2 or rng.random() < 0.5) else 3
        h = int(rng.integers(0, n_seen - k + 1)) if n_seen > k else 0
        for i in range(h, min(h + k, n_seen)):
            c = Rs[i].T @ (pts[j] - poses[i, :3])
            if c[2] > 0:
                m = np.array([fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy]) + rng.normal(0, noise_px, 2)
            else:
                m = np.array([cx, cy])
            node.append(i)
            point.append(j)
            uv.append(m)
    node, point, uv = np.array(node, np.int32), np.array(point, np.int32), np.array(uv)
    # repeats: three exact (no-ops), two with another keypoint (rejected)
    dup = rng.choice(len(node), 5, replace=False)
    d_uv = uv[dup].copy()
    d_uv[3:] += 7.0
    node = np.concatenate([node, node[dup]])
    point = np.concatenate([point, point[dup]])
    uv = np.concatenate([uv, d_uv])
    start_nodes = poses.copy()
    for i in range(1, n_nodes):
        start_nodes[i, :3] += rng.normal(0, 0.01, 3)
        dq = np.concatenate([[1.0], rng.normal(0, 0.002, 3)])
        q = synthetic.quat_mul(poses[i, 3:], dq)
        start_nodes[i, 3:] = q / np.linalg.norm(q)
    start_points = pts + rng.normal(0, 0.02, pts.shape)
    return dict(camera=CAMERA, true_nodes=poses, true_points=pts, nodes=start_nodes, points=start_points,
                node=node, point=point, uv=uv, scale=float(np.abs(pts).max()))


def oracle_system(scene):
    import sba_oracle as so
    s = so.SysSBA(scene["camera"])
    for p in scene["nodes"]:
        s.add_node(p)
    for x in scene["points"]:
        s.add_point(x)
    for ni, pi, m in zip(scene["node"], scene["point"], scene["uv"]):
        s.add_proj(int(ni), int(pi), m)
    return s
