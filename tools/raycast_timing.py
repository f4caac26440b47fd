"""Timing of the ray-casting kernels (k_tsdf_mean and k_tsdf_raycast behind ekf_raycast_render) on a 256^3 volume
with a 640 x 480 view and on a 128^3 volume with a 320 x 240 view, both at step voxel / 2.  The volume holds the analytic sphere
of tools/fusion_timing.py (radius 0.35 of the side); the camera stands at the origin and looks down +z through the whole
volume.  Per size: the mean HIP-event time of each kernel over --reps renders after three warm-up renders (ekf_fusion_profile;
the mean plane is made again for every render because the volume is marked changed in between), the pixels that hit, the
nominal samples per second (width x height x N over the time of k_tsdf_raycast; the samples a ray skips outside the box or
after its hit are counted, so the figure compares runs of this tool only), and as a reference point the mean time of
k_tsdf_integrate over the same volume in the same session with the map of tools/fusion_timing.py.  No gate: the parent has no
such path.
Usage: python tools/raycast_timing.py [--reps 50] [--out profiles/raycast_timing_mi355x.json]"""
import argparse, json, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools")]
from __graft_entry__ import load_package
from fusion_timing import wall_map


def run(pkg, n, w, h, reps):
    voxel = 2.56 / n
    origin = np.array([-1.28, -1.28, 1.0]) + 0.5 * voxel
    v = pkg.TsdfVolume((n, n, n), origin, voxel, 4 * voxel)
    pose = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    depth, img, K = wall_map(w, h, 0.8 * w, 2.28)
    for _ in range(3):
        v.integrate_host(depth, img, K, pose)
    v.reset()
    v.profile(True)
    for _ in range(reps):
        v.integrate_host(depth, img, K, pose)
    integrate_ms = v.get_profile()["k_tsdf_integrate"][0] / reps
    v.profile(False)
    x = origin[0] + np.arange(n, dtype=np.float64) * voxel
    z = origin[2] + np.arange(n, dtype=np.float64) * voxel
    c = (x[0] + x[-1]) / 2, (z[0] + z[-1]) / 2
    dist = np.sqrt((x[None, None, :] - c[0]) ** 2 + (x[None, :, None] - c[0]) ** 2 + (z[:, None, None] - c[1]) ** 2) - 0.35 * 2.56
    v.set_volume(np.clip(dist / (4 * voxel), -1, 1).astype(np.float32), np.ones((n, n, n), np.uint16), np.full((n, n, n), 128, np.uint32))
    z_near, z_far, step = 0.9, 3.7, voxel / 2
    samples = int(np.floor((z_far - z_near) / step)) + 1
    call = lambda: v._check(v._lib.ekf_raycast_render(v._h, w, h, K.ctypes.data, pose.ctypes.data, z_near, z_far, step, 1))
    for _ in range(3):
        r = v.raycast((w, h), K, pose, z_near, z_far, step, 1)
    v.profile(True)
    for _ in range(reps):
        v.set_volume()                                             # no plane given: only marks the volume changed
        call()                                                     # (no copy of the images to the host)
    prof = v.get_raycast_profile()
    v.profile(False)
    assert all(prof[k][1] == reps for k in prof), prof
    ms = prof["k_tsdf_raycast"][0] / reps
    row = {"volume": "%d^3" % n, "view": "%d x %d" % (w, h), "reps": reps, "step": step, "samples_per_ray": samples,
           "pixels_hit": int((r.depth > 0).sum()), "k_tsdf_mean_ms": prof["k_tsdf_mean"][0] / reps, "k_tsdf_raycast_ms": ms,
           "nominal_samples_per_s": w * h * samples / (ms * 1e-3), "k_tsdf_integrate_ms": integrate_ms}
    v.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = load_package()
    rows = [run(pkg, 256, 640, 480, a.reps), run(pkg, 128, 320, 240, a.reps)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/raycast_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
