"""Views shared by tests/test_oracle_raycast.py, tests/test_gpu_raycast.py and tools/raycast_host_check.py;
tests/fusion_scene.py and tests/dense_scene.py are imported read-only.

The sphere shape looks at the analytic sphere of fusion_scene (17 x 15 x 13 voxels of 0.25, radius 1.25 about the origin)
through a 29 x 23 view: 2 x 2 workgroups of 16 x 16 pixels, the right and the bottom ones partly outside the image.  Pose A
is on the axis, pose B off it and rotated.  Steps of 0.125 and 0.25 (half a voxel, a voxel) hit the whole silhouette; a step
of 0.4 lets rays step over the rim of the sphere (an inside-to-outside pair) or meet their first valid sample inside it.
The main shape renders the integrated 19 x 13 x 11 volume at two of the poses it was fused from, 37 x 19 pixels: voxels
without a count break pairs, and min_count 1, 2, 3 give fewer and at last no hits.
"""
import numpy as np

import dense_scene as ds
import fusion_oracle as fo
import fusion_scene as fs

SPHERE_SHAPE = (29, 23)
SPHERE_K = np.array([30.0, 30.0, 14.0, 11.0], np.float64)
SPHERE_NEAR, SPHERE_FAR = 2.0, 6.5
POSE_A = np.array([0.0, 0.0, -4.0, 1.0, 0.0, 0.0, 0.0], np.float64)
POSE_B = ds._pose([0.9, -0.4, -3.8], [0.08, -0.2, 0.05])
SPHERE_STEPS = (0.125, 0.25, 0.4)
AWAY = np.array([0.0, 0.0, -4.0, 0.0, 1.0, 0.0, 0.0], np.float64)     # half a turn about x: the camera looks along -z

MAIN_SHAPE = (fs.MAP_W, fs.MAP_H)
MAIN_NEAR, MAIN_STEP, MAIN_N = 0.05, 0.05, 24
MAIN_FAR = MAIN_NEAR + (MAIN_N - 0.5) * MAIN_STEP                    # N = floor(23.5) + 1 = 24
MAIN_COUNTS = (1, 2, 3)


def sphere_case(pose, step, z_near=SPHERE_NEAR, shape=SPHERE_SHAPE, K=SPHERE_K, vol=None):
    return dict(vol=fs.sphere_volume() if vol is None else vol, dims=fs.SPHERE_DIMS, origin=fs.SPHERE_ORIGIN, voxel=fs.SPHERE_VOXEL,
                shape=shape, K=K, pose=pose, z_near=z_near, z_far=SPHERE_FAR, step=step, min_count=1)


def main_case(vol, n, min_count):
    return dict(vol=vol, dims=fs.DIMS, origin=fs.ORIGIN, voxel=fs.VOXEL, shape=MAIN_SHAPE, K=fs.K_MAP, pose=fs.POSES[n],
                z_near=MAIN_NEAR, z_far=MAIN_FAR, step=MAIN_STEP, min_count=min_count)


def cases():
    """{name: the keyword arguments of raycast_oracle.raycast} of every exact case."""
    out = {}
    sphere = fs.sphere_volume()
    for s, step in enumerate(SPHERE_STEPS):
        out["sphere_A_step%d" % s] = sphere_case(POSE_A, step, vol=sphere)
        out["sphere_B_step%d" % s] = sphere_case(POSE_B, step, vol=sphere)
    out["sphere_A_near4"] = sphere_case(POSE_A, 0.125, z_near=4.0, vol=sphere)
    out["sphere_away"] = sphere_case(AWAY, 0.125, vol=sphere)
    out["sphere_1x1"] = sphere_case(POSE_A, 0.125, shape=(1, 1), K=np.array([30.0, 30.0, 0.0, 0.0]), vol=sphere)
    main = fs.fused()[0][-1]
    for n in (0, 1):
        for mc in MAIN_COUNTS:
            out["main_%d_min%d" % (n, mc)] = main_case(main, n, mc)
    out["empty"] = main_case(fo.empty_volume(fs.DIMS), 0, 1)
    return out


def oracle_audit_from_recording(read_recording, neighbours_of, directory, nodes_out=None, voxel=None, bounds=None, trunc=None,
                                min_count=2, neighbours=2, w_min=0.05, w_max=2.0, planes=64, radius=2, trunc_cost=40, rel_tol=0.01,
                                min_agree=1):
    """audit_recording restated on the oracles, from the same files: (z_near, z_far, step, [per key frame dict(render,
    overlap, median, p90, grey_error)])."""
    import dense_oracle as do
    import raycast_oracle as ro
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
    z = np.concatenate([d[d > 0].astype(np.float64) for d in depth])
    z_near, z_far, step = max(0.0, float(z.min()) - float(tr)), float(z.max()) + float(tr), vx / 2.0
    h, w = images[0].shape
    frames = []
    for i in range(n):
        r = ro.raycast(vol, dims, origin, vx, (w, h), K, poses[i], z_near, z_far, step, min_count)
        both, hit = (r["depth"] > 0) & (depth[i] > 0), r["depth"] > 0
        rel = np.abs(r["depth"][both].astype(np.float64) - depth[i][both].astype(np.float64)) / depth[i][both].astype(np.float64)
        frames.append(dict(render=r, overlap=float(both.mean()), median=float(np.median(rel)), p90=float(np.percentile(rel, 90)),
                           grey_error=float(np.abs(r["grey"][hit].astype(np.float64) - images[i][hit].astype(np.float64)).mean())))
    return z_near, z_far, step, frames
