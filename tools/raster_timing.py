"""The figures of DESIGN.md §30.4.

Fidelity, on the CPU with tests/raster_oracle.py: the painted sphere of tools/texture_timing.py and its six views.  For the weld and
for its simplification at 1, 2 and 4 voxels the mesh is textured from the six views (P = 8, 1 channel) and rasterised at each
view's pose with shading 0 (vertex colours) and shading 1 (the atlas); the mean absolute grey error against the view's own image
over the pixels both hit, and, beside it, the median and the 90th percentile of |raster depth - ray-cast depth| in voxels over
the pixels both renders hit.  Reported whichever way they fall.

Kernel times, on the device: the 256^3 sphere of tools/mesh_timing.py, its weld and its simplifications at 2 and 4 voxels, one
640 x 480 view, both shadings, culling on, at small_limit 16, 64 and 256.  Per kernel the median of --reps runs with the range
(ekf_fusion_profile switched on anew before every run, after three warm-up runs), beside k_tsdf_raycast of the same view in the
same session, and the wall time of a render with the copies of its images.  No gate: the parent has none of this.
Usage: python tools/raster_timing.py [--fidelity-only] [--reps 50] [--n 256] [--out profiles/raster_timing_mi355x.json]"""
import argparse, json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tools"), os.path.join(R, "tests")]
import raster_oracle as ro
import texture_oracle as to
from texture_timing import PATCH, paint, painted_view, stats

FACTORS = (2.0, 4.0)
LIMITS = (16, 64, 256)


def fidelity(view_width=232):
    import fusion_oracle as fo
    import fusion_scene as fs
    import mesh_oracle as mo
    import raycast_oracle as rc
    import raycast_scene as rsc
    import simplify_oracle as so
    import texture_scene as ts
    s, c, _ = fs.sphere_volume()
    P = fo.centres(fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL)
    vol = (s, c, np.floor(paint(np.stack(P, axis=3)) + 0.5).astype(np.uint32))
    _, key, _, _ = fo.extract(vol, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, 1)
    weld = mo.weld(vol, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, key, 1, False)
    scale = view_width / float(ts.W)
    shape = (int(ts.W * scale), int(ts.H * scale))
    K = np.array([ts.K[0] * scale, ts.K[1] * scale, (ts.K[2] + 0.5) * scale - 0.5, (ts.K[3] + 0.5) * scale - 0.5])
    views = [dict(image=painted_view(shape, K, pose, 1.25), K=K, pose=pose) for pose in ts.AXES]
    cast = [rc.raycast(vol, fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, shape, K, pose, rsc.SPHERE_NEAR, rsc.SPHERE_FAR,
                       fs.SPHERE_VOXEL / 2.0, 1)["depth"] for pose in ts.AXES]
    rows = []
    for factor in (None, 1.0, 2.0, 4.0):
        m = weld if factor is None else so.as_mesh(so.simplify(weld, fs.SPHERE_ORIGIN, fs.SPHERE_DIMS, fs.SPHERE_VOXEL, factor * fs.SPHERE_VOXEL))
        atlas = to.texture(m, PATCH, 1, views)["atlas"]
        err, diff, hits = {0: [], 1: []}, [], 0
        for v, z in zip(views, cast):
            for shading in (0, 1):
                r = ro.rasterise(m, shape, K, v["pose"], 0.0, True, atlas if shading else None, PATCH if shading else None)
                both = (r["tri"] >= 0) & (v["image"] > 0)
                err[shading].append(np.abs(r["grey"][both].astype(np.float64) - v["image"][both].astype(np.float64)))
            seen = (r["tri"] >= 0) & (z > 0)
            diff.append(np.abs(r["depth"][seen].astype(np.float64) - z[seen].astype(np.float64)) / fs.SPHERE_VOXEL)
            hits += int((r["tri"] >= 0).sum())
        diff = np.concatenate(diff)
        row = {"mesh": "weld" if factor is None else "simplified at %g voxels" % factor, "triangles": len(m["faces"]),
               "vertices": len(m["vertices"]), "view_shape": list(shape), "views": len(views), "patch": PATCH, "hit_pixels": hits,
               "mean_abs_grey_error_shading_0": float(np.concatenate(err[0]).mean()),
               "mean_abs_grey_error_shading_1": float(np.concatenate(err[1]).mean()),
               "depth_minus_raycast_voxels_median": float(np.median(diff)), "depth_minus_raycast_voxels_p90": float(np.percentile(diff, 90))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


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
    rows = []
    for factor in (None,) + FACTORS:
        source = "weld" if factor is None else "simplified"
        m = v.weld(1) if factor is None else v.simplify(factor * voxel)
        v.texture_begin(source, PATCH, 1)
        v.texture_add_view_host(image, K, pose)
        v.texture_finish()
        for shading in ("vertex", "texture"):
            for limit in LIMITS:
                v.set_raster_small_limit(limit)
                once = lambda: v.rasterise((W, H), K, pose, source, 0.0, True, shading)
                for _ in range(3):
                    got = once()
                kinds = {k: [] for k in v.get_raster_profile()}
                rays = []
                for _ in range(reps):
                    v.profile(True)
                    once()
                    for k, (t, _) in v.get_raster_profile().items():
                        kinds[k].append(t)
                    v.raycast((W, H), K, pose, 1.0, 3.6)
                    rays.append(v.get_raycast_profile()["k_tsdf_raycast"][0])
                v.profile(False)
                wall = []
                for _ in range(max(3, reps // 5)):
                    t0 = time.perf_counter()
                    once()
                    wall.append(time.perf_counter() - t0)
                row = {"volume": "sphere %d^3" % n, "source": source if factor is None else "simplified at %g voxels" % factor,
                       "shading": shading, "small_limit": limit, "reps": reps, "triangles": len(m.faces), "vertices": len(m.key),
                       "view": [W, H], "hit_pixels": int((got.tri >= 0).sum())}
                row.update({k + "_ms": stats(ts_) for k, ts_ in kinds.items()})
                row["k_tsdf_raycast_ms"] = stats(rays)
                row["render_wall_with_the_copies_s"] = stats(wall)
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
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = {"tool": "tools/raster_timing.py"}
    if not a.device_only:
        out["fidelity"] = fidelity(a.view_width)
    if not a.fidelity_only:
        from __graft_entry__ import load_package
        out["results"] = device(load_package(), a.n, a.reps)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
