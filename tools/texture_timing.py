"""The two sets of figures of DESIGN.md §29.4.

Fidelity, on the CPU with tests/texture_oracle.py: the analytic sphere of tests/fusion_scene.py (17 x 15 x 13 voxels of 0.25,
radius 1.25) painted with a procedural grey f(X); the volume's grey plane is f at the voxel centres, so the weld's vertex grey is
what fusion would have given it; six views on the axes (tests/texture_scene.py's AXES, --view-width pixels wide), each image f at
the hit point of the pixel's ray on the analytic sphere.  For the weld and for its simplification at 1, 2 and 4 voxels: the mean
absolute error of the atlas against f at every textured texel's 3D point pushed radially onto the sphere, and beside it the same
error of the barycentric blend of the mesh's own vertex grey at the same texels.  Both columns are reported whichever way they
fall.

Kernel times, on the device: the 256^3 sphere of tools/mesh_timing.py, its weld and its simplifications at 2 and 4 voxels, P = 8,
one 640 x 480 view behind a ray cast of the volume.  Per kernel the median of --reps runs with the range (ekf_fusion_profile
switched on anew before every run, after three warm-up runs), beside k_tsdf_raycast and the weld's five launches of the same
session; the wall time of begin + view + finish with the copy of the atlas; the bytes to the host with and without the atlas;
the host baseline, the vectorised oracle on the copied mesh and image (not for the weld: its 45 M texels take the oracle several
GB), which the device's result must equal bit for bit.  No gate: the parent has none of this.
Usage: python tools/texture_timing.py [--fidelity-only] [--reps 50] [--n 256] [--out profiles/texture_timing_mi355x.json]"""
import argparse, json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools"), os.path.join(R, "tests")]
import texture_oracle as to

FACTORS = (2.0, 4.0)
PATCH = 8


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def paint(X):
    """The procedural grey of a point, 28 .. 228: periods of 1.26, 0.90 and 2.09 units (5, 3.6 and 8.4 voxels of 0.25)."""
    X = np.asarray(X, np.float64)
    return 128.0 + 60.0 * np.sin(5.0 * X[..., 0]) + 40.0 * np.cos(7.0 * X[..., 1]) * np.sin(3.0 * X[..., 2])


def painted_view(shape, K, pose, radius):
    """f at the hit point of every pixel's ray on the sphere of ``radius`` round the origin; 0 where the ray misses."""
    import dense_oracle as do
    w, h = shape
    t, q = do.normalise_pose(pose)
    Rm = do.rotation(q)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    dc = np.stack([(x - K[2]) / K[0], (y - K[3]) / K[1], np.ones_like(x)], axis=2)
    dw = dc @ Rm.T
    a, b, c = (dw * dw).sum(axis=2), 2.0 * (dw @ t), t @ t - radius * radius
    disc = b * b - 4.0 * a * c
    s = (-b - np.sqrt(np.maximum(disc, 0.0))) / (2.0 * a)
    hit = (disc > 0.0) & (s > 0.0)
    return np.where(hit, np.floor(paint(t + s[:, :, None] * dw) + 0.5), 0.0).astype(np.uint8)


def fidelity(view_width=232):
    import fusion_oracle as fo
    import fusion_scene as fs
    import mesh_oracle as mo
    import simplify_oracle as so
    import texture_scene as ts
    s, c, _ = fs.sphere_volume()
    P = fo.centres(fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL)
    g = np.floor(paint(np.stack(P, axis=3)) + 0.5).astype(np.uint32)
    vol = (s, c, g)
    _, key, _, _ = fo.extract(vol, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1)
    weld = mo.weld(vol, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, key, 1, False)
    scale = view_width / float(ts.W)
    shape = (int(ts.W * scale), int(ts.H * scale))
    K = np.array([ts.K[0] * scale, ts.K[1] * scale, (ts.K[2] + 0.5) * scale - 0.5, (ts.K[3] + 0.5) * scale - 0.5])
    views = [dict(image=painted_view(shape, K, pose, 1.25), K=K, pose=pose) for pose in ts.AXES]
    rows = []
    for factor in (None, 1.0, 2.0, 4.0):
        m = weld if factor is None else so.as_mesh(so.simplify(weld, fs.SPHERE_ORIGIN, fs.SPHERE_DIMS, fs.SPHERE_VOXEL, factor * fs.SPHERE_VOXEL))
        X, F, grey = np.asarray(m["vertices"]), np.asarray(m["faces"], np.int64), np.asarray(m["grey"], np.float64)
        r = to.texture(m, PATCH, 1, views)
        tri, l0, l1, l2 = to.texel_map(len(F), PATCH)
        sel = np.zeros(tri.shape, bool)
        sel[tri >= 0] = r["view"][tri[tri >= 0]] >= 0
        ty, tx = np.nonzero(sel)
        f = F[tri[ty, tx]]
        a0, a1, a2 = l0[ty, tx][:, None], l1[ty, tx][:, None], l2[ty, tx][:, None]
        Xp = (a0 * X[f[:, 0]] + a1 * X[f[:, 1]]) + a2 * X[f[:, 2]]
        Xs = 1.25 * Xp / np.sqrt((Xp * Xp).sum(axis=1))[:, None]
        truth = paint(Xs)
        blend = np.clip(np.floor(((a0[:, 0] * grey[f[:, 0]] + a1[:, 0] * grey[f[:, 1]]) + a2[:, 0] * grey[f[:, 2]]) + 0.5), 0, 255)
        row = {"mesh": "weld" if factor is None else "simplified at %g voxels" % factor, "triangles": len(F), "vertices": len(X),
               "textured_triangles": r["n_textured"], "textured_texels": int(len(ty)), "atlas_side": int(r["atlas"].shape[0]),
               "view_shape": list(shape), "views": len(views), "patch": PATCH,
               "mean_abs_error_of_the_atlas": float(np.abs(r["atlas"][ty, tx, 0].astype(np.float64) - truth).mean()),
               "mean_abs_error_of_the_vertex_blend": float(np.abs(blend - truth).mean())}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def mesh_bytes(nv, nt):
    return nv * (24 + 8 + 1) + nt * 12


def device(pkg, n, reps):
    from mesh_timing import sphere_planes
    voxel = 2.56 / n
    origin = np.array([-1.28, -1.28, 1.0]) + 0.5 * voxel
    v = pkg.TsdfVolume((n, n, n), origin, voxel, 4 * voxel)
    v.set_volume(*sphere_planes(n, voxel, origin))
    W, H = 640, 480
    K = np.array([500.0, 500.0, 319.5, 239.5])
    pose = np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    image = ((x * 7 + y * 13) % 256).astype(np.uint8)
    occ = (1.0, 3.6, None, 1)
    welds = []
    for i in range(3 + reps):
        v.set_volume()                                               # no plane given: only marks the volume changed
        v.profile(True)
        v.weld(1)
        if i >= 3:
            welds.append(sum(t for t, _ in v.get_mesh_profile().values()))
    v.profile(False)
    rows = []
    for factor in (None,) + FACTORS:
        source = "weld" if factor is None else "simplified"
        m = v.weld(1) if factor is None else v.simplify(factor * voxel)
        nv, nt = len(m.key), len(m.faces)
        tol = voxel if factor is None else factor * voxel

        def once():
            v.texture_begin(source, PATCH, 1)
            won = v.texture_add_view_host(image, K, pose, occ, tol)
            return v.texture_finish(), won

        for _ in range(3):
            got, won = once()
        kinds = {k: [] for k in v.get_texture_profile()}
        rays = []
        for _ in range(reps):
            v.profile(True)
            once()
            for k, (t, _) in v.get_texture_profile().items():
                kinds[k].append(t)
            rays.append(v.get_raycast_profile()["k_tsdf_raycast"][0])
        v.profile(False)
        wall = []
        for _ in range(max(3, reps // 5)):
            t0 = time.perf_counter()
            once()
            wall.append(time.perf_counter() - t0)
        side = got.atlas.shape[0]
        row = {"volume": "sphere %d^3" % n, "source": source if factor is None else "simplified at %g voxels" % factor, "reps": reps,
               "triangles": nt, "vertices": nv, "patch": PATCH, "atlas_side": side, "view": [W, H], "triangles_won": won,
               "triangles_textured": got.n_textured}
        row.update({k + "_ms": stats(ts_) for k, ts_ in kinds.items()})
        row["k_tsdf_raycast_ms"] = stats(rays)
        row["weld_kernels_ms"] = stats(welds)
        row["begin_view_finish_wall_with_the_atlas_copy_s"] = stats(wall)
        row["bytes_to_host_without_the_atlas"] = mesh_bytes(nv, nt)
        row["bytes_to_host_with_the_atlas"] = mesh_bytes(nv, nt) + side * side + nt * 48
        if factor is not None:                                       # the host baseline, and the bits
            src = dict(vertices=m.vertices, faces=m.faces, grey=m.grey, colour=None)
            z = v._render().depth
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                want = to.texture(src, PATCH, 1, [dict(image=image, K=K, pose=pose, zbuf=z, tol=tol)])
                host.append(time.perf_counter() - t0)
            row["host_oracle_after_the_copy_s"] = stats(host)
            row["equals_the_oracle_bit_for_bit"] = bool(np.array_equal(got.atlas, want["atlas"][:, :, 0]) and np.array_equal(got.view, want["view"]) and
                                                        np.array_equal(got.score.view(np.uint64), want["score"].view(np.uint64)))
        rows.append(row)
        print(json.dumps(row), flush=True)
    v.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--view-width", type=int, default=232)
    ap.add_argument("--fidelity-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"tool": "tools/texture_timing.py", "fidelity": fidelity(a.view_width)}
    if not a.fidelity_only:
        from __graft_entry__ import load_package
        out["results"] = device(load_package(), a.n, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
