"""Timing of the TSDF fusion kernels (k_tsdf_integrate behind ekf_fusion_integrate*, k_tsdf_count / k_tsdf_scan /
k_tsdf_emit behind ekf_fusion_extract) at 256^3 with a 640 x 480 map and at 128^3 with a 320 x 240 map.  Per size: the mean
HIP-event time of k_tsdf_integrate over --reps launches after three warm-up launches (ekf_fusion_profile), the share of
voxels a launch updates, and the bytes it actually moves (20 B per updated voxel: 10 in, 10 out) over that time as a
fraction of the device copy rate that tools/copy_bw_probe.py reaches in the same session (its best "full" line); then, on an
injected analytic sphere of the same size, the mean time of each extraction kernel and the triangle count.  No gate: the
parent has no such path.
Usage: python tools/fusion_timing.py [--reps 50] [--out profiles/fusion_timing_mi355x.json]"""
import argparse, ctypes, json, os, re, subprocess, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R]
from __graft_entry__ import load_package


def copy_rate():
    """Bytes per second (read + write) of the best full copy of tools/copy_bw_probe.py, run as a process of its own."""
    out = subprocess.run([sys.executable, os.path.join(R, "tools", "copy_bw_probe.py")], capture_output=True, text=True, check=True).stdout
    rates = [float(m) for m in re.findall(r"^full .*?([0-9.]+) TB/s", out, flags=re.M)]
    return max(rates) * 1e12


def wall_map(w, h, f, z):
    X, Y = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    depth = (z + 0.02 * np.sin(0.05 * X) * np.cos(0.07 * Y)).astype(np.float32)
    img = ((X * 3 + Y * 5) % 256).astype(np.uint8)
    return depth, img, np.array([f, f, (w - 1) / 2.0, (h - 1) / 2.0])


def run(pkg, n, w, h, reps, bw):
    voxel = 2.56 / n
    origin = np.array([-1.28, -1.28, 1.0]) + 0.5 * voxel
    v = pkg.TsdfVolume((n, n, n), origin, voxel, 4 * voxel)
    # a camera at the origin looking down +z at a rippled wall through the middle of the volume; the frustum covers about
    # two thirds of the volume's width at the wall
    depth, img, K = wall_map(w, h, 0.8 * w, 2.28)
    pose = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)
    for _ in range(3):
        v.integrate_host(depth, img, K, pose)
    v.reset()
    v.profile(True)
    for _ in range(reps):
        v.integrate_host(depth, img, K, pose)
    prof = v.get_profile()
    v.profile(False)
    assert prof["k_tsdf_integrate"][1] == reps, prof
    updated = int(v.volume()["cnt"].astype(np.int64).sum()) // reps            # every launch updates the same voxels
    ms = prof["k_tsdf_integrate"][0] / reps
    row = {"volume": "%d^3" % n, "map": "%d x %d" % (w, h), "reps": reps, "k_tsdf_integrate_ms": ms,
           "voxels_updated_share": updated / float(n) ** 3, "bytes_moved": 20 * updated,
           "bytes_per_s": 20 * updated / (ms * 1e-3), "fraction_of_copy_rate": 20 * updated / (ms * 1e-3) / bw}
    # the extraction on a sphere of radius 0.35 of the side
    x = origin[0] + np.arange(n, dtype=np.float64) * voxel
    z = origin[2] + np.arange(n, dtype=np.float64) * voxel
    c = (x[0] + x[-1]) / 2, (z[0] + z[-1]) / 2
    dist = np.sqrt((x[None, None, :] - c[0]) ** 2 + (x[None, :, None] - c[0]) ** 2 + (z[:, None, None] - c[1]) ** 2) - 0.35 * 2.56
    v.set_volume(np.clip(dist / (4 * voxel), -1, 1).astype(np.float32), np.ones((n, n, n), np.uint16), np.full((n, n, n), 128, np.uint32))
    for _ in range(3):
        mesh = v.extract(1)
    v.profile(True)
    ntri = 0
    cnt = ctypes.c_ulonglong(0)
    for _ in range(reps):
        v._check(v._lib.ekf_fusion_extract(v._h, 1, ctypes.byref(cnt)))      # (no copy of the mesh to the host)
        ntri = int(cnt.value)
    prof = v.get_profile()
    v.profile(False)
    assert ntri == len(mesh.xyz) and all(prof[k][1] == reps for k in ("k_tsdf_count", "k_tsdf_scan", "k_tsdf_emit")), prof
    row.update({"sphere_triangles": ntri, "k_tsdf_count_ms": prof["k_tsdf_count"][0] / reps, "k_tsdf_scan_ms": prof["k_tsdf_scan"][0] / reps,
                "k_tsdf_emit_ms": prof["k_tsdf_emit"][0] / reps})
    v.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bw = copy_rate()
    pkg = load_package()
    rows = [run(pkg, 256, 640, 480, a.reps, bw), run(pkg, 128, 320, 240, a.reps, bw)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/fusion_timing.py", "copy_bytes_per_s": bw, "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
