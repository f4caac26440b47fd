"""Timing of the mesh smoothing on the device in one session on two 256^3 volumes: the analytic sphere of
tools/mesh_timing.py and the wave volume of tests/mesh_scene.py at min_count 2.  Per kernel: the mean HIP-event time over --reps
rounds after three warm-up rounds (ekf_fusion_profile), a round being smooth(10, normals=True) and components() on a fresh weld,
so that every round builds the adjacency; from them the adjacency build as a whole, one step with the bytes a second it
achieves against the bytes it must move (the neighbour indices, the gathered rows, one row read and one written, and the
8 bytes a vertex that say where its list lies and how long it is), ten rounds and the normals; beside them the weld's five
launches and k_comp_union of the same session; the wall time and the bytes to the host of weld() + smooth() beside weld() alone
(profiling off, the volume marked changed before each); and the host alternative on the same faces: a scipy.sparse Laplacian
built once and applied 20 times, with the copy of the weld it needs (where scipy does not import: tests/smooth_oracle.py's
vectorised step, with a note saying so).  No gate: the parent has none of this.
Usage: python tools/smooth_timing.py [--reps 20] [--n 256] [--out profiles/smooth_timing_mi355x.json]"""
import argparse, json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools"), os.path.join(R, "tests")]
from __graft_entry__ import load_package
from mesh_timing import sphere_planes

ADJACENCY = ("k_smooth_count", "k_smooth_offsets", "k_tsdf_scan", "k_smooth_fill", "k_smooth_lists")


def host_alternative(weld, lam, mu):
    """(seconds to build, seconds for 20 applications, what) of ten rounds on the host."""
    f = weld.faces.astype(np.int64)
    nv = len(weld.key)
    try:
        from scipy.sparse import coo_matrix, identity
    except ImportError:
        import smooth_oracle as so
        t0 = time.perf_counter()
        adj = so.adjacency(f, nv)
        t1 = time.perf_counter()
        X = weld.vertices
        for _ in range(10):
            X = so.step(so.step(X, adj, lam), adj, mu)
        return t1 - t0, time.perf_counter() - t1, "tests/smooth_oracle.py's vectorised step (scipy does not import)"
    t0 = time.perf_counter()
    rows = np.concatenate([f[:, a] for a in range(3) for b in range(3) if a != b])
    cols = np.concatenate([f[:, b] for a in range(3) for b in range(3) if a != b])
    A = coo_matrix((np.ones(len(rows)), (rows, cols)), shape=(nv, nv)).tocsr()
    A.data[:] = 1.0                                                  # an edge of two triangles counts once
    deg = np.asarray(A.sum(axis=1)).reshape(-1)
    W = A.multiply(1.0 / deg[:, None]).tocsr() - identity(nv, format="csr")      # mean of the neighbours - X
    t1 = time.perf_counter()
    X = weld.vertices
    for _ in range(10):
        X = X + lam * (W @ X)
        X = X + mu * (W @ X)
    return t1 - t0, time.perf_counter() - t1, "a scipy.sparse Laplacian on the same faces (no fixed order of summation: not the contract's bits)"


def run_volume(pkg, name, n, planes, voxel, origin, reps, min_count):
    v = pkg.TsdfVolume((n, n, n), origin, voxel, 4 * voxel)
    v.set_volume(*planes)
    weld = v.weld(min_count)
    for _ in range(3):
        v.set_volume()                                               # no plane given: only marks the volume changed
        v.weld(min_count)
        v.smooth(10, normals=True)
        adj = v.adjacency()
        v.components()
    v.profile(True)
    for _ in range(reps):
        v.set_volume()
        v.weld(min_count)
        v.smooth(10, normals=True)
        v.components()
    sp, cp, mp = v.get_smooth_profile(), v.get_component_profile(), v.get_mesh_profile()
    v.profile(False)
    per = {k: 1 for k in ADJACENCY}
    per.update({"k_smooth_step": 20, "k_smooth_normals": 1})
    assert all(sp[k][1] == reps * c for k, c in per.items()), sp
    alone, both = [], []
    for _ in range(max(3, reps // 4)):
        v.set_volume()
        t0 = time.perf_counter()
        v.weld(min_count)
        t1 = time.perf_counter()
        v.set_volume()
        t2 = time.perf_counter()
        v.weld(min_count)
        v.smooth(10, normals=True)
        t3 = time.perf_counter()
        alone.append(t1 - t0)
        both.append(t3 - t2)
    nv, nt, links = len(weld.key), len(weld.faces), int(adj.deg.astype(np.int64).sum())
    row = {"volume": "%s %d^3" % (name, n), "min_count": min_count, "reps": reps, "triangles": nt, "vertices": nv,
           "boundary_vertices": int(adj.boundary.sum()), "longest_incident_list": int(adj.inc.max()), "longest_neighbour_list": int(adj.deg.max())}
    row.update({(k if k != "k_tsdf_scan" else "k_tsdf_scan_of_the_adjacency") + "_ms": t / c for k, (t, c) in sp.items()})
    row["adjacency_kernels_ms"] = sum(sp[k][0] / sp[k][1] for k in ADJACENCY)
    row["step_bytes"] = links * (4 + 24) + nv * (24 + 24 + 8)
    row["step_gb_per_s"] = row["step_bytes"] / (row["k_smooth_step_ms"] * 1e-3) / 1e9
    row["ten_rounds_ms"] = 20 * row["k_smooth_step_ms"]
    row["weld_kernels_ms"] = sum(t for t, _ in mp.values()) / reps
    row["k_comp_union_ms"] = cp["k_comp_union"][0] / cp["k_comp_union"][1]
    row["weld_wall_s"] = float(np.median(alone))
    row["weld_and_smooth_wall_s"] = float(np.median(both))
    row["weld_bytes_to_host"] = nv * (24 + 8 + 1) + nt * 12
    row["weld_and_smooth_bytes_to_host"] = row["weld_bytes_to_host"] + nv * (24 + 8 + 1 + 12) + nt * 12
    row["host_build_s"], row["host_20_steps_s"], row["host_alternative"] = host_alternative(weld, 0.5, -0.53)
    row["host_copy_s"] = row["weld_wall_s"]
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
            json.dump({"tool": "tools/smooth_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
