"""Scenes and shapes shared by tests/test_oracle_colour.py, tests/test_gpu_colour.py and tools/colour_host_check.py
(DESIGN.md §18.5).  The shapes are those of the grey tests: tests/dense_scene.py, tests/fusion_scene.py and
tests/raycast_scene.py are imported read-only, and only the images are new.

Images are deterministic: pattern(w, h, n)[y, x, c] = (7 x + 13 y + 101 c + 29 n) % 256, constant images, images with
B = G = R, and for the recording a scene-consistent tint of the wall's texture.
"""
import os

import numpy as np

import colour_oracle as co
import dense_oracle as do
import dense_scene as ds
import fusion_oracle as fo
import fusion_scene as fs
import raycast_scene as rsc

# k_bgr_to_grey: pixel counts 2867 and 703 are 3 mod 4 (a byte-wise tail of 3; three workgroups and one), 48 x 32 = 1536 is a
# multiple of the 4 pixels of a lane (no tail); 1 x 1 and 2 x 1 have no full group at all, 5 x 1 has one and a tail of 1
GREY_SHAPES = ((ds.W, ds.H), (ds.SMALL_W, ds.SMALL_H), (fs.REC_W, fs.REC_H))
TINY_GREY_SHAPES = ((1, 1), (2, 1), (5, 1))
CONSTANT = (17, 201, 94)                                          # B, G, R

HOST_CHECK_CASES = ("main_min1", "main_min2", "main_min4", "tiny", "sphere", "mixed", "empty")


def pattern(w, h, n=0):
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing="ij")
    return ((x * 7 + y * 13 + c * 101 + n * 29) % 256).astype(np.uint8)


def constant(w, h, bgr=CONSTANT):
    return np.broadcast_to(np.array(bgr, np.uint8), (h, w, 3)).copy()


def tint(grey):
    """A colour image from a grey one, channel by channel a function of the grey value (so that views of one scene agree):
    B = g, G = g // 2 + 64, R = g // 2.  Its grey conversion keeps more than half of the contrast."""
    g = np.asarray(grey, np.uint8)
    return np.stack([g, g // 2 + 64, g // 2], axis=2).astype(np.uint8)


def colour_maps(kind="pattern"):
    """The three synthetic maps of fusion_scene with a colour image each: (depth, bgr, K, pose)."""
    out = []
    for n, (depth, img, K, pose) in enumerate(fs.synthetic_maps()):
        h, w = depth.shape
        bgr = {"pattern": lambda: pattern(w, h, n), "constant": lambda: constant(w, h), "tint": lambda: tint(img),
               "equal": lambda: np.repeat(img[:, :, None], 3, axis=2)}[kind]()
        out.append((depth, bgr, K, pose))
    return out


def fused(dims=fs.DIMS, origin=fs.ORIGIN, maps=None, order=(0, 1, 2)):
    """The oracle's colour volume after each map in turn and the classes of every map."""
    maps = colour_maps() if maps is None else maps
    vol = co.empty_volume(dims)
    steps, classes = [], []
    for n in order:
        classes.append(co.integrate(vol, dims, origin, fs.VOXEL, fs.TRUNC, *maps[n]))
        steps.append(tuple(p.copy() for p in vol))
    return steps, classes


def sphere_volume(kind="pattern"):
    """fusion_scene's analytic sphere with three colour planes: cnt = 1 everywhere, so a plane is its voxels' colour."""
    s, c, g = fs.sphere_volume()
    nx, ny, nz = fs.SPHERE_DIMS
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    if kind == "equal":
        cs = np.stack([g, g, g])
    elif kind == "constant":
        cs = np.stack([np.full(s.shape, v, np.uint32) for v in CONSTANT])
    else:
        cs = np.stack([((i * 7 + j * 13 + k * 29 + ch * 101) % 256).astype(np.uint32) for ch in range(3)])
    return s, c, g, cs.astype(np.uint32)


def raycast_cases():
    """{name: the keyword arguments of colour_oracle.raycast}: the sphere views of raycast_scene and its main case."""
    sphere = sphere_volume()
    out = {"sphere_A": rsc.sphere_case(rsc.POSE_A, 0.125, vol=sphere), "sphere_B": rsc.sphere_case(rsc.POSE_B, 0.25, vol=sphere),
           "sphere_away": rsc.sphere_case(rsc.AWAY, 0.125, vol=sphere)}
    main = fused()[0][-1]
    out["main_0_min1"] = rsc.main_case(main, 0, 1)
    out["main_1_min2"] = rsc.main_case(main, 1, 2)
    return out


# ---- a small rectified colour recording of the textured wall, as KeyframeRecorder(rectify=True, images=True) writes it from a
# 3-channel raw selector: fusion_scene's wall recording with <id>.ppm images
def write_colour_recording(directory, formats, write_ppm):
    os.makedirs(directory, exist_ok=True)
    formats.write_camera(os.path.join(directory, "camera.txt"), fs.REC_K)
    ids = [4 + 3 * i for i in range(fs.REC_N)]
    with open(os.path.join(directory, "nodes_and_prjcts.txt"), "w") as fh:
        for i, kid in enumerate(ids):
            pose = ds._pose([0.12 * (i - 2), 0.01 * (i % 2), 0.0], [0.0, 0.004 * (i - 2), 0.002 * i]).astype(np.float32)
            fh.write(formats.pose_record(kid, pose, None))
            img, _ = ds.render(pose.astype(np.float64), ("plane", fs.REC_Z), Kc=fs.REC_K, w=fs.REC_W, h=fs.REC_H)
            write_ppm(os.path.join(directory, "%d.ppm" % kid), tint(img))
    return ids


def oracle_audit_from_recording(read_recording, neighbours_of, directory, nodes_out=None, voxel=None, bounds=None, trunc=None,
                                min_count=2, neighbours=2, w_min=0.05, w_max=2.0, planes=64, radius=2, trunc_cost=40, rel_tol=0.01,
                                min_agree=1):
    """audit_recording of a colour recording restated on the oracles, from the same files: dict(vertices, faces, grey, colour,
    origin, dims, voxel, trunc, z_near, z_far, step, frames = [dict(render, overlap, median, p90, grey_error, colour_error)]).
    The sweep and the filter see the grey conversion of every key frame; the volume is a colour volume."""
    K, ids, poses, images = read_recording(directory, nodes_out)
    greys = [co.grey_of(im) for im in images]
    n = len(ids)
    near = [neighbours_of(i, n, neighbours) for i in range(n)]
    swept = [do.sweep(greys[i], K, poses[i], [(greys[j], K, poses[j]) for j in near[i]], w_min, w_max, planes, radius, trunc_cost)
             for i in range(n)]
    depth = [do.geometric_filter(swept[i]["depth"], swept[i]["plane"], K, poses[i], [(swept[j]["depth"], K, poses[j]) for j in near[i]],
                                 rel_tol, min(min_agree, len(near[i])))[0] for i in range(n)]
    origin, dims, vx, tr = fo.auto_grid([do.points(depth[i], K, poses[i]) for i in range(n)], voxel, bounds, trunc)
    vol = co.empty_volume(dims)
    for i in range(n):
        co.integrate(vol, dims, origin, vx, tr, depth[i], images[i], K, poses[i])
    xyz, key, grey, colour = co.extract(vol, dims, origin, vx, min_count)
    first, faces = fo.weld(key)
    z = np.concatenate([d[d > 0].astype(np.float64) for d in depth])
    z_near, z_far, step = max(0.0, float(z.min()) - float(tr)), float(z.max()) + float(tr), vx / 2.0
    h, w = greys[0].shape
    frames = []
    for i in range(n):
        r = co.raycast(vol, dims, origin, vx, (w, h), K, poses[i], z_near, z_far, step, min_count)
        both, hit = (r["depth"] > 0) & (depth[i] > 0), r["depth"] > 0
        rel = np.abs(r["depth"][both].astype(np.float64) - depth[i][both].astype(np.float64)) / depth[i][both].astype(np.float64)
        frames.append(dict(render=r, depth=depth[i], overlap=float(both.mean()), median=float(np.median(rel)),
                           p90=float(np.percentile(rel, 90)),
                           grey_error=float(np.abs(r["grey"][hit].astype(np.float64) - greys[i][hit].astype(np.float64)).mean()),
                           colour_error=float(np.abs(r["colour"][hit].astype(np.float64)
                                                     - images[i][hit].astype(np.float64)).mean(axis=1).mean())))
    return dict(vertices=xyz.reshape(-1, 3)[first], faces=faces, grey=grey.reshape(-1)[first], colour=colour.reshape(-1, 3)[first],
                origin=origin, dims=tuple(int(v) for v in dims), voxel=vx, trunc=tr, z_near=z_near, z_far=z_far, step=step,
                frames=frames)
