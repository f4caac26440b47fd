"""Writes the case files tools/colour_host_check.cpp reads: the GPU test shapes of tests/colour_scene.py with the inputs and
the outputs of tests/colour_oracle.py.  Usage: python tools/colour_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import colour_oracle as co
import colour_scene as cs
import fusion_scene as fs
import raycast_oracle as ro
import raycast_scene as rsc


def write(path, dims, origin, voxel, trunc, maps, start, min_count, views=(), images=()):
    """ints nx ny nz n_maps min_count n_views n_images; doubles origin voxel trunc; per map ints W H channels, doubles K pose,
    the depth, the image (channels = 3: B G R, 1: a map without colour); the four planes before the maps; the oracle: the four
    planes after them, n_tri (uint64) and the vertex colours; per view ints W H N, doubles K pose z_near step, the oracle's
    depth, normal, grey and colour; per image int npix, the B G R bytes and the oracle's grey bytes."""
    vol = tuple(p.copy() for p in start)
    with open(path, "wb") as fh:
        fh.write(np.array(list(dims) + [len(maps), min_count, len(views), len(images)], np.int32).tobytes())
        fh.write(np.array(list(origin) + [voxel, trunc], np.float64).tobytes())
        for depth, img, K, pose in maps:
            img = np.ascontiguousarray(img, np.uint8)
            fh.write(np.array([depth.shape[1], depth.shape[0], 3 if img.ndim == 3 else 1], np.int32).tobytes())
            fh.write(np.asarray(K, np.float64).tobytes() + np.asarray(pose, np.float64).tobytes())
            fh.write(np.ascontiguousarray(depth, np.float32).tobytes() + img.tobytes())
        for p in vol:
            fh.write(p.tobytes())
        for m in maps:
            co.integrate(vol, dims, origin, voxel, trunc, *m)
        for p in vol:
            fh.write(p.tobytes())
        _, key, _, colour = co.extract(vol, dims, origin, voxel, min_count)
        fh.write(np.array([len(key)], np.uint64).tobytes() + colour.tobytes())
        hits = 0
        for shape, K, pose, z_near, z_far, step in views:
            r = co.raycast(vol, dims, origin, voxel, shape, K, pose, z_near, z_far, step, min_count)
            fh.write(np.array(list(shape) + [r["stats"]["samples"]], np.int32).tobytes())
            fh.write(np.array(list(K) + list(pose) + [z_near, step], np.float64).tobytes())
            fh.write(r["depth"].tobytes() + r["normal"].tobytes() + r["grey"].tobytes() + r["colour"].tobytes())
            hits += r["stats"]["hits"]
        for bgr in images:
            bgr = np.ascontiguousarray(bgr, np.uint8)
            fh.write(np.array([bgr.shape[0] * bgr.shape[1]], np.int32).tobytes() + bgr.tobytes() + co.grey_of(bgr).tobytes())
    print(os.path.basename(path), len(key), "triangles,", hits, "hits")


def main(out):
    os.makedirs(out, exist_ok=True)
    maps = cs.colour_maps()
    main_view = lambda n: (rsc.MAIN_SHAPE, fs.K_MAP, fs.POSES[n], rsc.MAIN_NEAR, rsc.MAIN_FAR, rsc.MAIN_STEP)
    sphere_view = lambda pose, step: (rsc.SPHERE_SHAPE, rsc.SPHERE_K, pose, rsc.SPHERE_NEAR, rsc.SPHERE_FAR, step)
    images = [cs.pattern(w, h, 1) for w, h in cs.GREY_SHAPES + cs.TINY_GREY_SHAPES]
    for mc in (1, 2, 4):
        write(os.path.join(out, "main_min%d.bin" % mc), fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC, maps, co.empty_volume(fs.DIMS), mc,
              [main_view(0), main_view(1)], images if mc == 1 else ())
    write(os.path.join(out, "tiny.bin"), fs.TINY_DIMS, fs.TINY_ORIGIN, fs.VOXEL, fs.TRUNC, maps, co.empty_volume(fs.TINY_DIMS), 1)
    write(os.path.join(out, "sphere.bin"), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, fs.SPHERE_TRUNC, [], cs.sphere_volume(), 1,
          [sphere_view(rsc.POSE_A, 0.125), sphere_view(rsc.POSE_B, 0.25), sphere_view(rsc.AWAY, 0.125)])
    grey = fs.synthetic_maps()
    write(os.path.join(out, "mixed.bin"), fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC, [maps[0], grey[1], maps[2]],
          co.empty_volume(fs.DIMS), 1, [main_view(0)])
    write(os.path.join(out, "empty.bin"), fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC, [], co.empty_volume(fs.DIMS), 1, [main_view(0)])


if __name__ == "__main__":
    main(sys.argv[1])
