"""Timing of the mesh-to-mesh distance on the device on the 256^3 sphere of tools/mesh_timing.py, in one session:
its weld (905 232 triangles) against its simplifications at cells of 2 and 4 voxels, in both directions, with the grid at g = 16,
32, 64, 128 and automatic (and g = 1, brute force on the device, only with --brute, once, for the 4-voxel pair: it takes seconds).
Per kernel: the median HIP-event time over --reps runs after two warm-up runs (ekf_fusion_profile), with the range; the cells,
the entries and the longest cell list of each setting; the arrays of every setting are compared with those of the first.  Beside
it the weld's five launches, and the vectorised oracle of tests/distance_oracle.py on the host after the copy, on --oracle-points
of the query points (the whole query would take hours).  No gate: the parent has no such path.
Usage: python tools/distance_timing.py [--reps 50] [--n 256] [--brute] [--out profiles/distance_timing_mi355x.json]"""
import argparse, json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools"), os.path.join(R, "tests")]

GRIDS = (16, 32, 64, 128, 0)
FACTORS = (2.0, 4.0)


def stats(ts):
    ts = sorted(ts)
    return {"median": ts[len(ts) // 2], "min": ts[0], "max": ts[-1]}


def same(a, b):
    return all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ("dist", "tri", "closest", "side"))


def run(pkg, n, reps, brute, oracle_points):
    import distance_oracle as do
    from mesh_timing import sphere_planes
    voxel = 2.56 / n
    origin = np.array([-1.28, -1.28, 1.0]) + 0.5 * voxel
    v = pkg.TsdfVolume((n, n, n), origin, voxel, 4 * voxel)
    v.set_volume(*sphere_planes(n, voxel, origin))
    rows = []
    for _ in range(3):
        v.set_volume()
        weld = v.weld(1)
    welds = {k: [] for k in v.get_mesh_profile()}
    for _ in range(reps):
        v.set_volume()
        v.profile(True)
        v.weld(1)
        for k, (t, _) in v.get_mesh_profile().items():
            welds[k].append(t)
    v.profile(False)
    row = {"volume": "sphere %d^3" % n, "what": "the weld's five launches", "triangles": len(weld.faces), "vertices": len(weld.key), "reps": reps}
    row.update({k + "_ms": stats(t) for k, t in welds.items()})
    row["sum_of_medians_ms"] = sum(stats(t)["median"] for t in welds.values())
    rows.append(row)
    print(json.dumps(row), flush=True)
    for factor in FACTORS:
        simp = v.simplify(factor * voxel)
        for target, query in (("weld", "simplified"), ("simplified", "weld")):
            first = None
            for g in ((1,) if brute and factor == FACTORS[-1] else ()) + GRIDS:
                v.set_distance_grid(g)
                n_rep = 1 if g == 1 else reps
                for _ in range(0 if g == 1 else 2):
                    v.distance(target, query)
                kinds = {k: [] for k in v.get_distance_profile()}
                for _ in range(n_rep):
                    v.profile(True)
                    got = v.distance(target, query)
                    st = v.distance_stats(voxel)
                    for k, (t, _) in v.get_distance_profile().items():
                        kinds[k].append(t)
                v.profile(False)
                first = first or got
                wall = []
                for _ in range(1 if g == 1 else max(3, reps // 5)):
                    t0 = time.perf_counter()
                    v.distance(target, query)
                    wall.append(time.perf_counter() - t0)
                grid = v.distance_grid()
                row = {"volume": "sphere %d^3" % n, "target": target, "query": query, "simplified_at_voxels": factor, "g": g or "automatic",
                       "reps": n_rep, "target_triangles": len((weld if target == "weld" else simp).faces), "points": len(got.dist),
                       "cells": grid["cells"], "entries": grid["entries"], "longest_cell_list": grid["longest"],
                       "identical_to_the_first_setting": bool(same(got, first)),
                       "max": st.max, "mean": st.mean, "rms": st.rms, "within_one_voxel": st.within, "n": st.n}
                row.update({k + "_ms": stats(t) for k, t in kinds.items()})
                row["run_kernels_sum_of_medians_ms"] = sum(stats(kinds[k])["median"] for k in list(kinds)[:7])
                row["run_wall_with_the_copies_s"] = stats(wall)
                rows.append(row)
                print(json.dumps(row), flush=True)
            # the vectorised oracle on the host after the copy, on a few of the query points
            src = {"weld": weld, "simplified": simp}
            tm, qm = src[target], src[query]
            idx = np.linspace(0, len(qm.vertices) - 1, oracle_points).astype(int)
            t0 = time.perf_counter()
            want = do.distance(dict(vertices=tm.vertices, faces=tm.faces), qm.vertices[idx], chunk=2 if target == "weld" else 8)
            oracle_s = time.perf_counter() - t0
            row = {"volume": "sphere %d^3" % n, "target": target, "query": query, "simplified_at_voxels": factor, "what": "the vectorised oracle on the host",
                   "points": int(oracle_points), "of_points": len(qm.vertices), "oracle_s": oracle_s,
                   "equal_to_the_device": bool(want["dist"].tobytes() == first.dist[idx].tobytes() and want["tri"].tobytes() == first.tri[idx].tobytes())}
            rows.append(row)
            print(json.dumps(row), flush=True)
    v.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--brute", action="store_true")
    ap.add_argument("--oracle-points", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from __graft_entry__ import load_package
    out = {"tool": "tools/distance_timing.py", "results": run(load_package(), a.n, a.reps, a.brute, a.oracle_points)}
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
