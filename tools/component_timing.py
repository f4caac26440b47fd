"""Timing of the mesh components on the device in one session on two 256^3 volumes: the analytic sphere of
tools/mesh_timing.py (one component: the worst case for the shared root) and the wave volume of tests/mesh_scene.py (many
fragments).  Per kernel: the mean HIP-event time over --reps rounds after three warm-up rounds (ekf_fusion_profile), a round
being components(), prune(9) and prune(largest=True) on a fresh weld; beside them the weld's five launches and k_tsdf_emit of
the same session; the wall time and the bytes to the host of weld() + prune(9) beside weld() alone (profiling off, the volume
marked changed before each); and the host alternative on the same faces: scipy.sparse.csgraph.connected_components where scipy
imports, else tests/component_oracle.py on a smaller volume, with a note saying so.  No gate: the parent has none of this.
Usage: python tools/component_timing.py [--reps 20] [--n 256] [--out profiles/component_timing_mi355x.json]"""
import argparse, json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools"), os.path.join(R, "tests")]
from __graft_entry__ import load_package
from mesh_timing import sphere_planes


def host_alternative(pkg, faces, n_vert, small):
    """(seconds, what) of labelling the components of `faces` on the host."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        import component_oracle as co
        m = small()
        t0 = time.perf_counter()
        co.components(m.faces, len(m.key))
        return time.perf_counter() - t0, "tests/component_oracle.py (scipy does not import) on a smaller volume of %d triangles" % len(m.faces)
    t0 = time.perf_counter()
    f = faces.astype(np.int64)
    rows, cols = np.concatenate([f[:, 0], f[:, 0]]), np.concatenate([f[:, 1], f[:, 2]])
    connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(n_vert, n_vert)), directed=False)
    return time.perf_counter() - t0, "scipy.sparse.csgraph.connected_components on the same faces (labels only: no sizes, no pruned mesh)"


def run_volume(pkg, name, n, planes, voxel, origin, reps, min_count):
    v = pkg.TsdfVolume((n, n, n), origin, voxel, 4 * voxel)
    v.set_volume(*planes)
    weld = v.weld(min_count)
    rounds = lambda: (v.components(), v.prune(9), v.prune(largest=True))
    for _ in range(3):
        v.set_volume()                                               # no plane given: only marks the volume changed
        v.weld(min_count)
        comp, cut, one = rounds()
    v.profile(True)
    for _ in range(reps):
        v.set_volume()
        v.weld(min_count)
        rounds()
    cp, mp, fp = v.get_component_profile(), v.get_mesh_profile(), v.get_profile()
    v.profile(False)
    per = {"k_comp_init": 1, "k_comp_union": 1, "k_comp_count": 1, "k_comp_largest": 1, "k_comp_flags": 3, "k_tsdf_scan": 6,
           "k_comp_vertices": 2, "k_comp_faces": 2}
    assert all(cp[k][1] == reps * c for k, c in per.items()), cp
    alone, both = [], []
    for _ in range(max(3, reps // 4)):
        v.set_volume()
        t0 = time.perf_counter()
        v.weld(min_count)
        t1 = time.perf_counter()
        v.set_volume()
        t2 = time.perf_counter()
        v.weld(min_count)
        v.prune(9)
        t3 = time.perf_counter()
        alone.append(t1 - t0)
        both.append(t3 - t2)
    row = {"volume": "%s %d^3" % (name, n), "min_count": min_count, "reps": reps, "triangles": len(weld.faces), "vertices": len(weld.key),
           "components": comp.count, "triangles_after_prune_9": len(cut.faces), "triangles_of_the_largest": len(one.faces)}
    row.update({(k if k != "k_tsdf_scan" else "k_tsdf_scan_of_a_prune_one_launch") + "_ms": t / c for k, (t, c) in cp.items()})
    row["components_kernels_ms"] = sum(cp[k][0] / cp[k][1] for k in ("k_comp_init", "k_comp_union", "k_comp_count"))
    row["prune_kernels_ms"] = (cp["k_comp_flags"][0] / cp["k_comp_flags"][1] + 3 * cp["k_tsdf_scan"][0] / cp["k_tsdf_scan"][1] +
                               cp["k_comp_vertices"][0] / cp["k_comp_vertices"][1] + cp["k_comp_faces"][0] / cp["k_comp_faces"][1])
    row["weld_kernels_ms"] = sum(t for t, _ in mp.values()) / reps
    row["k_tsdf_emit_ms"] = fp["k_tsdf_emit"][0] / reps
    row["union_costs_more_than_the_weld"] = bool(row["k_comp_union_ms"] > row["weld_kernels_ms"])
    row["weld_wall_s"] = float(np.median(alone))
    row["weld_and_prune_9_wall_s"] = float(np.median(both))
    row["weld_bytes_to_host"] = len(weld.key) * (24 + 8 + 1) + len(weld.faces) * 12
    row["weld_and_prune_9_bytes_to_host"] = row["weld_bytes_to_host"] + len(cut.key) * (24 + 8 + 1) + len(cut.faces) * 12

    def small():
        s = pkg.TsdfVolume((64, 64, 64), origin, voxel, 4 * voxel)
        s.set_volume(*(p[:64, :64, :64] for p in planes))
        try:
            return s.weld(min_count)
        finally:
            s.close()

    row["host_alternative_s"], row["host_alternative"] = host_alternative(pkg, weld.faces, len(weld.key), small)
    v.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import mesh_scene as ms
    pkg = load_package()
    n, voxel = a.n, 2.56 / a.n
    origin = np.array([-1.28, -1.28, 1.0]) + 0.5 * voxel
    rows = [run_volume(pkg, "sphere", n, sphere_planes(n, voxel, origin), voxel, origin, a.reps, 1),
            run_volume(pkg, "wave", n, ms.wave_volume((n, n, n), 0), voxel, origin, a.reps, 2)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/component_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
