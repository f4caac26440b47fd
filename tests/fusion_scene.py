"""Scenes and shapes shared by tests/test_oracle_fusion.py, tests/test_gpu_fusion.py and tools/fusion_host_check.py
(DESIGN.md §16.5); tests/dense_scene.py is imported read-only.

The main volume is 19 x 13 x 11: 2717 voxels and 18 x 12 x 10 = 2160 cells, neither a multiple of the 256 of a workgroup,
and 9 blocks of cells, so the block offsets of the extraction matter.  It is fed from three 37 x 19 maps of a rippled wall
near z = 0.55, each with holes, seen by a camera of short focal length (so that the frustum is wider than the volume near
the wall and narrower near the camera: every class of voxel occurs).  The sphere volume is 17 x 15 x 13 with the centre on
a voxel and a radius of 5 voxels: the 30 lattice points (±5, 0, 0), (±3, ±4, 0) and their permutations are exactly on it.
"""
import numpy as np

import dense_scene as ds
import fusion_oracle as fo

DIMS = (19, 13, 11)
ORIGIN = np.array([-0.95, -0.65, -0.15], np.float64)
VOXEL, TRUNC = 0.1, 0.25
MAP_W, MAP_H = ds.SMALL_W, ds.SMALL_H
K_MAP = np.array([24.0, 24.0, 18.0, 9.0], np.float64)
WALL_Z = 0.55
POSES = [ds.REF,
         ds._pose([0.2, 0.0, -0.05], [0.0, -0.08, 0.01]),
         ds._pose([-0.15, 0.05, 0.0], [0.03, 0.06, -0.02])]

TINY_DIMS = (2, 2, 2)
TINY_ORIGIN = np.array([-0.05, -0.05, 0.5], np.float64)

SPHERE_DIMS = (17, 15, 13)
SPHERE_VOXEL, SPHERE_TRUNC, SPHERE_RADIUS = 0.25, 0.5, 1.25
SPHERE_ORIGIN = np.array([-2.0, -1.75, -1.5], np.float64)          # the centre (0, 0, 0) is voxel (8, 7, 6)

# the cases tools/fusion_host_check.py writes: the main volume at three min_count, the one-cell volume, the sphere, no maps
HOST_CHECK_CASES = ("main_min1", "main_min2", "main_min4", "tiny", "sphere", "empty")


def synthetic_map(n):
    """(depth float32 with holes, image uint8, K, pose) of map n = 0, 1, 2."""
    img, z = ds.render(POSES[n], ("plane", WALL_Z), Kc=K_MAP, w=MAP_W, h=MAP_H)
    X, Y = np.meshgrid(np.arange(MAP_W, dtype=np.float64), np.arange(MAP_H, dtype=np.float64))
    depth = (z + 0.03 * np.sin(0.7 * X + 0.3 * Y + n)).astype(np.float32)
    depth[3 + n:8 + n, 20 - 4 * n:27 - 4 * n] = 0.0                  # a block without depth
    depth[(X.astype(int) * 7 + Y.astype(int) * 3 + n) % 11 == 0] = 0.0   # and scattered pixels
    return depth, img, K_MAP, POSES[n]


def synthetic_maps():
    return [synthetic_map(n) for n in range(3)]


def fused(dims=DIMS, origin=ORIGIN, maps=None, order=(0, 1, 2)):
    """The oracle's volume after each map in turn, and the classes of every map: ([(sum, cnt, gsum) after map], [classes])."""
    maps = synthetic_maps() if maps is None else maps
    vol = fo.empty_volume(dims)
    steps, classes = [], []
    for n in order:
        classes.append(fo.integrate(vol, dims, origin, VOXEL, TRUNC, *maps[n]))
        steps.append(tuple(p.copy() for p in vol))
    return steps, classes


def sphere_volume():
    """(sum, cnt, gsum) of the analytic sphere: the distance scaled by 1 / trunc and clamped, cnt = 1 everywhere."""
    X, Y, Z = fo.centres(SPHERE_DIMS, SPHERE_ORIGIN, SPHERE_VOXEL)
    dist = np.sqrt(X * X + Y * Y + Z * Z) - SPHERE_RADIUS
    s = np.clip(dist / SPHERE_TRUNC, -1.0, 1.0).astype(np.float32)
    nx, ny, nz = SPHERE_DIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return s, np.ones(s.shape, np.uint16), ((i * 7 + j * 13 + k * 29) % 256).astype(np.uint32)


# ---- the accuracy condition: the plane scene of tests/dense_scene.py, true depth maps from three poses -------------------------
ACC_Z = ds.plane_z(ds.TRUE_PLANE)
ACC_VOXEL = 0.125                                                 # 2.1 pixel footprints (Z / fx = 0.0593) at the plane
ACC_TRUNC = 4 * ACC_VOXEL
ACC_DIMS = (33, 27, 13)
ACC_ORIGIN = np.array([-2.0, -1.625, ACC_Z - 0.75], np.float64)
ACC_SLOTS = (0, 1, 2)


def accuracy_maps():
    out = []
    for s in ACC_SLOTS:
        img, z = ds.render(ds.RIG[s], ("plane", ACC_Z))
        out.append((z.astype(np.float32), img, ds.K, ds.RIG[s]))
    return out


def in_common_view(P, margin):
    """Which of the points P (m, 3) lie at least `margin` (world units) inside the image of every accuracy view."""
    import dense_oracle as do
    ok = np.ones(len(P), bool)
    for s in ACC_SLOTS:
        t, q = do.normalise_pose(ds.RIG[s])
        p = (P - t) @ do.rotation(q)
        m = margin * ds.K[0] / p[:, 2]
        sx, sy = ds.K[0] * p[:, 0] / p[:, 2] + ds.K[2], ds.K[1] * p[:, 1] / p[:, 2] + ds.K[3]
        ok &= (p[:, 2] > 0) & (sx >= m) & (sx <= ds.W - 1 - m) & (sy >= m) & (sy <= ds.H - 1 - m)
    return ok


# ---- a small rectified recording of the textured wall z = 2, written as KeyframeRecorder(rectify=True, images=True) writes it ----
REC_W, REC_H, REC_N = 48, 32, 5
REC_K = np.array([48.0, 48.0, 23.5, 15.5], np.float64)
REC_Z = 2.0
REC_SWEEP = dict(neighbours=1, w_min=0.3, w_max=0.7, planes=9, radius=2, trunc=60, rel_tol=0.1, min_agree=1)


def write_wall_recording(directory, formats, write_pgm):
    """camera.txt, nodes_and_prjcts.txt and the P5 images of REC_N key frames on a sideways line; returns their ids."""
    import os
    os.makedirs(directory, exist_ok=True)
    formats.write_camera(os.path.join(directory, "camera.txt"), REC_K)
    ids = [4 + 3 * i for i in range(REC_N)]
    with open(os.path.join(directory, "nodes_and_prjcts.txt"), "w") as fh:
        for i, kid in enumerate(ids):
            pose = ds._pose([0.12 * (i - 2), 0.01 * (i % 2), 0.0], [0.0, 0.004 * (i - 2), 0.002 * i]).astype(np.float32)
            fh.write(formats.pose_record(kid, pose, None))
            img, _ = ds.render(pose.astype(np.float64), ("plane", REC_Z), Kc=REC_K, w=REC_W, h=REC_H)
            write_pgm(os.path.join(directory, "%d.pgm" % kid), img)
    return ids


def oracle_mesh_from_recording(read_recording, neighbours_of, directory, nodes_out=None, voxel=None, bounds=None, trunc=None,
                               min_count=2, neighbours=2, w_min=0.05, w_max=2.0, planes=64, radius=2, trunc_cost=40, rel_tol=0.01,
                               min_agree=1):
    """mesh_from_recording restated on the oracles, from the same files: (vertices, faces, grey, origin, dims, voxel, trunc)."""
    import dense_oracle as do
    K, ids, poses, images = read_recording(directory, nodes_out)
    n = len(ids)
    near = [neighbours_of(i, n, neighbours) for i in range(n)]
    swept = [do.sweep(images[i], K, poses[i], [(images[j], K, poses[j]) for j in near[i]], w_min, w_max, planes, radius, trunc_cost)
             for i in range(n)]
    depth = [do.geometric_filter(swept[i]["depth"], swept[i]["plane"], K, poses[i], [(swept[j]["depth"], K, poses[j]) for j in near[i]],
                                 rel_tol, min(min_agree, len(near[i])))[0] for i in range(n)]
    origin, dims, vx, tr = fo.auto_grid([do.points(depth[i], K, poses[i]) for i in range(n)], voxel, bounds, trunc)
    vol = fo.empty_volume(dims)
    for i in range(n):
        fo.integrate(vol, dims, origin, vx, tr, depth[i], images[i], K, poses[i])
    xyz, key, grey, _ = fo.extract(vol, dims, origin, vx, min_count)
    first, faces = fo.weld(key)
    return xyz.reshape(-1, 3)[first], faces, grey.reshape(-1)[first], origin, tuple(int(v) for v in dims), vx, tr
