"""Writes the case files tools/fusion_host_check.cpp reads: the GPU test shapes of tests/fusion_scene.py with the inputs and
the outputs of tests/fusion_oracle.py.  Usage: python tools/fusion_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import fusion_oracle as fo
import fusion_scene as fs


def write(path, dims, origin, voxel, trunc, maps, start, min_count):
    """ints nx ny nz n_maps min_count; doubles origin voxel trunc; per map ints W H, doubles K pose, the depth, the image;
    the planes before the maps; the oracle: the planes after them, n_tri (uint64), xyz, key, grey."""
    vol = tuple(p.copy() for p in start)
    with open(path, "wb") as fh:
        fh.write(np.array(list(dims) + [len(maps), min_count], np.int32).tobytes())
        fh.write(np.array(list(origin) + [voxel, trunc], np.float64).tobytes())
        for depth, img, K, pose in maps:
            fh.write(np.array([depth.shape[1], depth.shape[0]], np.int32).tobytes())
            fh.write(np.asarray(K, np.float64).tobytes() + np.asarray(pose, np.float64).tobytes())
            fh.write(np.ascontiguousarray(depth, np.float32).tobytes() + np.ascontiguousarray(img, np.uint8).tobytes())
        for p in vol:
            fh.write(p.tobytes())
        for m in maps:
            fo.integrate(vol, dims, origin, voxel, trunc, *m)
        for p in vol:
            fh.write(p.tobytes())
        xyz, key, grey, _ = fo.extract(vol, dims, origin, voxel, min_count)
        fh.write(np.array([len(xyz)], np.uint64).tobytes() + xyz.tobytes() + key.tobytes() + grey.tobytes())
    print(os.path.basename(path), len(xyz), "triangles")


def main(out):
    os.makedirs(out, exist_ok=True)
    maps = fs.synthetic_maps()
    for mc in (1, 2, 4):
        write(os.path.join(out, "main_min%d.bin" % mc), fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC, maps, fo.empty_volume(fs.DIMS), mc)
    write(os.path.join(out, "tiny.bin"), fs.TINY_DIMS, fs.TINY_ORIGIN, fs.VOXEL, fs.TRUNC, maps, fo.empty_volume(fs.TINY_DIMS), 1)
    write(os.path.join(out, "sphere.bin"), fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, fs.SPHERE_TRUNC, [], fs.sphere_volume(), 1)
    write(os.path.join(out, "empty.bin"), fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC, [], fo.empty_volume(fs.DIMS), 1)


if __name__ == "__main__":
    main(sys.argv[1])
