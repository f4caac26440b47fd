"""Timing of the mesh simplification on the device in one session on two 256^3 volumes: the analytic sphere of
tools/mesh_timing.py and the wave volume of tests/mesh_scene.py at min_count 2, each at cells of 1, 2 and 4 voxels.  Per kind of
launch and for the kernels of a whole run: the median of --reps runs with the range (ekf_fusion_profile switched on anew before
every run, after three warm-up runs; k_tsdf_scan is the sum of a run's five); the wall time of a run with its copy to the host,
profiling off; beside them the weld's five launches of the same session (the median of --reps welds, the volume marked changed
before each) and the weld's wall time with its copy; the bytes to the host before (the weld) and after (the simplified mesh);
the host baseline: tests/simplify_oracle.py's vectorised form on the copied weld (the median of three), which the device's
result must equal bit for bit; and, on the sphere, the mean distance of the vertices from the analytic surface before and
after.  No gate: the parent has none of this.
Usage: python tools/simplify_timing.py [--reps 50] [--n 256] [--out profiles/simplify_timing_mi355x.json]"""
import argparse, json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools"), os.path.join(R, "tests")]
from __graft_entry__ import load_package
from mesh_timing import sphere_planes
import simplify_oracle as so

FACTORS = (1.0, 2.0, 4.0)


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def mesh_bytes(nv, nt):
    return nv * (24 + 8 + 1) + nt * 12


def same_bits(got, want):
    eq = lambda a, b: a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
    return bool(eq(got.vertices, want["vertices"]) and np.array_equal(got.faces, want["faces"]) and eq(got.grey, want["grey"]) and
                eq(got.key, want["key"]))


def run_volume(pkg, name, n, planes, voxel, origin, reps, min_count, sphere=None):
    v = pkg.TsdfVolume((n, n, n), origin, voxel, 4 * voxel)
    v.set_volume(*planes)
    weld = v.weld(min_count)
    nv, nt = len(weld.key), len(weld.faces)
    src = dict(vertices=weld.vertices, faces=weld.faces, grey=weld.grey, colour=None, normals=None, key=weld.key)
    # the weld's five launches and its wall time, in this session
    welds, weld_wall = [], []
    for i in range(3 + reps):
        v.set_volume()                                               # no plane given: only marks the volume changed
        v.profile(True)
        v.weld(min_count)
        if i >= 3:
            welds.append(sum(t for t, _ in v.get_mesh_profile().values()))
    v.profile(False)
    for _ in range(max(3, reps // 4)):
        v.set_volume()
        t0 = time.perf_counter()
        v.weld(min_count)
        weld_wall.append(time.perf_counter() - t0)
    rows = []
    for f in FACTORS:
        cell = f * voxel
        for _ in range(3):
            got = v.simplify(cell)
        kinds = {k: [] for k in v.get_simplify_profile()}
        whole = []
        for _ in range(reps):
            v.profile(True)
            v.simplify(cell)
            p = v.get_simplify_profile()
            for k, (t, _) in p.items():
                kinds[k].append(t)
            whole.append(sum(t for t, _ in p.values()))
        v.profile(False)
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            v.simplify(cell)
            wall.append(time.perf_counter() - t0)
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            want = so.simplify(src, origin, (n, n, n), voxel, cell)
            host.append(time.perf_counter() - t0)
        ov, ot = len(got.key), len(got.faces)
        occupied = int(len(np.unique(want["cells"])))
        row = {"volume": "%s %d^3" % (name, n), "min_count": min_count, "cell_voxels": f, "reps": reps, "grid": list(want["grid"]),
               "cells": int(np.prod(want["grid"])), "occupied_cells": occupied, "used_cells": ov,
               "longest_member_list": int(np.bincount(want["cells"]).max()),
               "triangles_before": nt, "triangles_after": ot, "vertices_before": nv, "vertices_after": ov,
               "degenerate": v.simplify_stats.degenerate, "duplicate": v.simplify_stats.duplicate,
               "equals_the_oracle_bit_for_bit": same_bits(got, want) and bool(np.array_equal(v.simplify_map(), want["map"]))}
        row.update({(k if k != "k_tsdf_scan" else "k_tsdf_scan_five_launches") + "_ms": stats(ts) for k, ts in kinds.items()})
        row["run_kernels_ms"] = stats(whole)
        row["run_wall_with_copy_s"] = stats(wall)
        row["weld_kernels_ms"] = stats(welds)
        row["weld_wall_with_copy_s"] = stats(weld_wall)
        row["bytes_to_host_before"] = mesh_bytes(nv, nt)
        row["bytes_to_host_after"] = mesh_bytes(ov, ot)
        row["host_oracle_after_the_copy_s"] = stats(host)
        if sphere is not None:
            centre, radius = sphere
            dist = lambda X: float(np.abs(np.sqrt(((X - centre) ** 2).sum(axis=1)) - radius).mean())
            row["mean_distance_from_the_sphere_before"] = dist(weld.vertices)
            row["mean_distance_from_the_sphere_after"] = dist(want["vertices"])
            row["mean_distance_in_voxels_before"] = row["mean_distance_from_the_sphere_before"] / voxel
            row["mean_distance_in_voxels_after"] = row["mean_distance_from_the_sphere_after"] / voxel
        rows.append(row)
        print(json.dumps(row), flush=True)
    v.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mesh_scene as ms
    pkg = load_package()
    n, voxel = a.n, 2.56 / a.n
    origin = np.array([-1.28, -1.28, 1.0]) + 0.5 * voxel
    x = origin[0] + np.arange(n, dtype=np.float64) * voxel
    z = origin[2] + np.arange(n, dtype=np.float64) * voxel
    centre = np.array([(x[0] + x[-1]) / 2, (x[0] + x[-1]) / 2, (z[0] + z[-1]) / 2])
    rows = run_volume(pkg, "sphere", n, sphere_planes(n, voxel, origin), voxel, origin, a.reps, 1, (centre, 0.35 * n * voxel))
    rows += run_volume(pkg, "wave", n, ms.wave_volume((n, n, n), 0), voxel, origin, a.reps, 2)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/simplify_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
