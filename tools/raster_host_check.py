"""Writes the case files tools/raster_host_check.cpp reads: the hand-built meshes of tests/raster_scene.py and the sphere's weld
with their view and the oracle's images.
Usage: python tools/raster_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import raster_oracle as ro
import raster_scene as rs
import texture_oracle as to
import texture_scene as ts


def cases():
    """name -> (mesh, shape, K, pose, z_near, cull, atlas or None, P)."""
    out = {}
    for name, (mesh, shape, z_near) in rs.scenes().items():
        out[name] = (mesh, shape, rs.K, rs.POSE, z_near, True, None, 0)
    out["fan_back"] = (dict(rs.fan(), faces=rs.fan()["faces"][:, ::-1].copy()), rs.FAN_SHAPE, rs.K, rs.POSE, 0.0, False, None, 0)
    out["clip_no_near"] = (rs.clip(), rs.CLIP_SHAPE, rs.K, rs.POSE, 0.0, False, None, 0)
    sphere = rs.sphere()
    out["sphere_B_both_sides"] = (sphere, (ts.W, ts.H), ts.K, ts.POSES[1], 0.0, False, None, 0)
    out["sphere_big"] = (sphere, rs.BIG_SHAPE, rs.BIG_K, ts.AXES[2], 0.0, True, None, 0)
    for P, channels in ((2, 3), (8, 1)):
        atlas = to.texture(sphere, P, channels, ts.views(True))["atlas"]
        out["sphere_atlas_p%d_c%d" % (P, channels)] = (sphere, (ts.W, ts.H), ts.K, ts.POSES[1], 0.0, True, atlas, P)
    return out


def names():
    return sorted(cases())


def write(path, mesh, shape, K, pose, z_near, cull, atlas, P):
    """ints n_vert n_tri has_bgr W H cull shading P C A colour; float64 K[4] pose7 z_near; the mesh: xyz, faces (uint32), grey,
    bgr; the atlas; then the oracle's depth, normal, grey, colour, tri, bary and cover."""
    r = ro.rasterise(mesh, shape, K, pose, z_near, cull, atlas, P or None, cover=True)
    X, F = np.ascontiguousarray(mesh["vertices"], np.float64), np.ascontiguousarray(mesh["faces"]).astype(np.uint32)
    bgr = mesh.get("colour") is not None
    C, A = (atlas.shape[2], atlas.shape[0]) if atlas is not None else (0, 0)
    with open(path, "wb") as fh:
        fh.write(np.array([len(X), len(F), bgr, shape[0], shape[1], cull, atlas is not None, P, C, A, r["colour"] is not None], np.int32).tobytes())
        fh.write(np.array(list(K) + list(pose) + [z_near], np.float64).tobytes())
        fh.write(X.tobytes() + F.tobytes() + np.ascontiguousarray(mesh["grey"], np.uint8).tobytes())
        if bgr:
            fh.write(np.ascontiguousarray(mesh["colour"], np.uint8).tobytes())
        if atlas is not None:
            fh.write(np.ascontiguousarray(atlas).tobytes())
        fh.write(r["depth"].tobytes() + r["normal"].tobytes() + r["grey"].tobytes())
        if r["colour"] is not None:
            fh.write(r["colour"].tobytes())
        fh.write(r["tri"].tobytes() + r["bary"].tobytes() + r["cover"].tobytes())
    print(os.path.basename(path), len(X), "vertices", len(F), "triangles,", shape, "pixels,", int((r["tri"] >= 0).sum()), "hit")


def main(out):
    os.makedirs(out, exist_ok=True)
    for name, case in cases().items():
        write(os.path.join(out, name + ".bin"), *case)


if __name__ == "__main__":
    main(sys.argv[1])
