"""Timing of the weld on the device beside the path it replaces, in one session on the 256^3 volume of
tools/fusion_timing.py's extraction (the analytic sphere of radius 0.35 of the side): the five launches of a weld beside
k_tsdf_emit, with and without normals; the wall time of extract() + weld() on the host beside TsdfVolume.weld() including its
copies; and the bytes each path moves to the host.  Per kernel: the mean HIP-event time over --reps welds after three warm-up
welds (ekf_fusion_profile); the wall times are taken with profiling off, the volume marked changed before each, so that
both paths extract.  No gate: the parent has no device weld.
Usage: python tools/mesh_timing.py [--reps 20] [--n 256] [--out profiles/mesh_timing_mi355x.json]"""
import argparse, json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools")]
from __graft_entry__ import load_package


def sphere_planes(n, voxel, origin):
    x = origin[0] + np.arange(n, dtype=np.float64) * voxel
    z = origin[2] + np.arange(n, dtype=np.float64) * voxel
    c = (x[0] + x[-1]) / 2, (z[0] + z[-1]) / 2
    dist = np.sqrt((x[None, None, :] - c[0]) ** 2 + (x[None, :, None] - c[0]) ** 2 + (z[:, None, None] - c[1]) ** 2) - 0.35 * n * voxel
    return np.clip(dist / (4 * voxel), -1, 1).astype(np.float32), np.ones((n, n, n), np.uint16), np.full((n, n, n), 128, np.uint32)


def run(pkg, n, reps):
    voxel = 2.56 / n
    origin = np.array([-1.28, -1.28, 1.0]) + 0.5 * voxel
    v = pkg.TsdfVolume((n, n, n), origin, voxel, 4 * voxel)
    v.set_volume(*sphere_planes(n, voxel, origin))
    rows = []
    for normals in (False, True):
        for _ in range(3):
            v.set_volume()                                         # no plane given: only marks the volume changed
            m = v.weld(1, normals)
        v.profile(True)
        for _ in range(reps):
            v.set_volume()
            v.weld(1, normals)
        mp, fp = v.get_mesh_profile(), v.get_profile()
        v.profile(False)
        assert all(c == reps for _, c in mp.values()) and fp["k_tsdf_emit"][1] == reps, (mp, fp)
        host_s, dev_s = [], []
        for _ in range(max(3, reps // 4)):
            v.set_volume()
            t0 = time.perf_counter()
            soup = v.extract(1)
            hv, hf, hg = pkg.weld(soup)
            t1 = time.perf_counter()
            v.set_volume()
            t2 = time.perf_counter()
            m = v.weld(1, normals)
            t3 = time.perf_counter()
            host_s.append(t1 - t0)
            dev_s.append(t3 - t2)
        assert np.array_equal(m.vertices, hv) and np.array_equal(m.faces, hf) and np.array_equal(m.grey, hg)
        n_tri, n_vert = len(m.faces), len(m.vertices)
        row = {"volume": "%d^3" % n, "normals": normals, "reps": reps, "triangles": n_tri, "vertices": n_vert,
               "k_tsdf_emit_ms": fp["k_tsdf_emit"][0] / reps}
        row.update({k + "_ms": t / reps for k, (t, _) in mp.items() if k != "k_tsdf_scan"})
        row["k_tsdf_scan_of_the_weld_ms"] = mp["k_tsdf_scan"][0] / reps
        row["weld_kernels_ms"] = sum(t for t, _ in mp.values()) / reps
        row["host_path_wall_s"] = float(np.median(host_s))          # extract() with its copies + np.unique on the host
        row["device_path_wall_s"] = float(np.median(dev_s))         # weld() with its extract, its launches and its copies
        row["host_path_bytes_to_host"] = n_tri * 3 * (24 + 8 + 1)
        row["device_path_bytes_to_host"] = n_vert * (24 + 8 + 1 + (12 if normals else 0)) + n_tri * 12
        rows.append(row)
    v.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = run(load_package(), a.n, a.reps)
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/mesh_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
