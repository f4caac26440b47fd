"""Timing of the three colour kernels of the fusion handle beside the grey kernels they run in place of or after,
in one session on a 256^3 volume with a 640 x 480 map and view: k_tsdf_integrate_colour beside k_tsdf_integrate,
k_tsdf_raycast_colour beside k_tsdf_raycast, k_tsdf_colour_vertices beside k_tsdf_emit.  The map is the wall of
tools/fusion_timing.py with a colour image, the rendered volume the analytic sphere of tools/raycast_timing.py at step
voxel / 2, the mesh that sphere's.  Per kernel: the mean HIP-event time over --reps launches after three warm-up launches
(ekf_fusion_profile).  For the integration it also states the bytes a voxel that is updated reads and writes: sum 4, cnt 2 and
gsum 4 in grey (10 and 10), and csum 3 x 4 more in colour (22 and 22); the map's depth and pixel come on top in both.  No gate:
the parent has no colour path.
Usage: python tools/colour_timing.py [--reps 50] [--n 256] [--out profiles/colour_timing_mi355x.json]"""
import argparse, ctypes as C, json, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools")]
from __graft_entry__ import load_package
from fusion_timing import wall_map


def run(pkg, colour, n, w, h, reps):
    voxel = 2.56 / n
    origin = np.array([-1.28, -1.28, 1.0]) + 0.5 * voxel
    v = pkg.TsdfVolume((n, n, n), origin, voxel, 4 * voxel, colour=colour)
    pose = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    depth, img, K = wall_map(w, h, 0.8 * w, 2.28)
    image = np.stack([img, img // 2 + 64, 255 - img], axis=2) if colour else img
    for _ in range(3):
        v.integrate_host(depth, image, K, pose)
    v.reset()
    v.profile(True)
    for _ in range(reps):
        v.integrate_host(depth, image, K, pose)
    integrate = (v.get_colour_profile()["k_tsdf_integrate_colour"] if colour else v.get_profile()["k_tsdf_integrate"])
    updated = int((v.volume()["cnt"] > 0).sum())
    v.profile(False)
    assert integrate[1] == reps, integrate
    x = origin[0] + np.arange(n, dtype=np.float64) * voxel
    z = origin[2] + np.arange(n, dtype=np.float64) * voxel
    c = (x[0] + x[-1]) / 2, (z[0] + z[-1]) / 2
    dist = np.sqrt((x[None, None, :] - c[0]) ** 2 + (x[None, :, None] - c[0]) ** 2 + (z[:, None, None] - c[1]) ** 2) - 0.35 * 2.56
    planes = dict(csum=np.stack([np.full((n, n, n), k, np.uint32) for k in (40, 128, 200)])) if colour else {}
    v.set_volume(np.clip(dist / (4 * voxel), -1, 1).astype(np.float32), np.ones((n, n, n), np.uint16), np.full((n, n, n), 128, np.uint32),
                 **planes)
    z_near, z_far, step = 0.9, 3.7, voxel / 2
    render = lambda: v._check(v._lib.ekf_raycast_render(v._h, w, h, K.ctypes.data, pose.ctypes.data, z_near, z_far, step, 1))
    n_tri = C.c_ulonglong(0)
    extract = lambda: v._check(v._lib.ekf_fusion_extract(v._h, 1, C.byref(n_tri)))           # (no copy of the mesh to the host)
    for _ in range(3):
        r = v.raycast((w, h), K, pose, z_near, z_far, step, 1)
        extract()
    v.profile(True)
    for _ in range(reps):
        v.set_volume()                                             # no plane given: only marks the volume changed
        render()
        extract()
    rp, fp, cp = v.get_raycast_profile(), v.get_profile(), v.get_colour_profile()
    v.profile(False)
    cast = cp["k_tsdf_raycast_colour"] if colour else rp["k_tsdf_raycast"]
    assert cast[1] == reps and fp["k_tsdf_emit"][1] == reps, (cast, fp)
    row = {"volume": "%d^3" % n, "view": "%d x %d" % (w, h), "colour": bool(colour), "reps": reps, "voxels_updated_per_map": updated,
           "pixels_hit": int((r.depth > 0).sum()), "triangles": int(n_tri.value),
           "integrate_kernel": "k_tsdf_integrate_colour" if colour else "k_tsdf_integrate", "integrate_ms": integrate[0] / reps,
           "bytes_read_per_updated_voxel": 22 if colour else 10, "bytes_written_per_updated_voxel": 22 if colour else 10,
           "raycast_kernel": "k_tsdf_raycast_colour" if colour else "k_tsdf_raycast", "raycast_ms": cast[0] / reps,
           "k_tsdf_mean_ms": rp["k_tsdf_mean"][0] / reps, "k_tsdf_emit_ms": fp["k_tsdf_emit"][0] / reps}
    if colour:
        assert cp["k_tsdf_colour_vertices"][1] == reps, cp
        row["k_tsdf_colour_vertices_ms"] = cp["k_tsdf_colour_vertices"][0] / reps
    v.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = load_package()
    rows = [run(pkg, False, a.n, 640, 480, a.reps), run(pkg, True, a.n, 640, 480, a.reps)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/colour_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
