"""Writes the case files tools/texture_host_check.cpp reads: meshes of tests/component_scene.py and tests/texture_scene.py with
their views and the oracle's atlas, views, scores and UVs.
Usage: python tools/texture_host_check.py OUT_DIR"""
import os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(R, "tests")]
import component_scene as cs
import texture_oracle as to
import texture_scene as ts


def one_triangle():
    """A mesh of one triangle that faces pose A."""
    return dict(vertices=np.array([[-0.5, -0.5, 0.0], [0.0, 0.6, 0.1], [0.7, -0.4, -0.1]]), faces=np.array([[0, 1, 2]]),
                grey=np.array([10, 200, 90], np.uint8), colour=None)


def cases():
    """name -> (mesh, P, channels, views)."""
    sphere = cs.oracle_mesh("sphere", 1)
    return {
        "sphere_p3_c3": (sphere, 3, 3, ts.views(True)),
        "sphere_p2_c1_grey": (sphere, 2, 1, ts.views(False)),
        "sphere_p5_c1_colour": (sphere, 5, 1, ts.views(True)),
        "main_p8_c3_grey": (cs.oracle_mesh("main", 1), 8, 3, ts.main_views(False, min_area2=0.5)),
        "wave_257x2x2_p5_c3": (cs.oracle_mesh("257x2x2", 1), 5, 3, ts.views(True)),
        "simplified_p32_c1": (ts.simplified("sphere", 1, 2.0), 32, 1, ts.views(False)),
        "occlusion_p4_c1": (ts.occlusion_mesh(), 4, 1, [ts.occlusion_view(True), ts.occlusion_view(False)]),
        "one_triangle_p2_c3": (one_triangle(), 2, 3, ts.views(True)),
        "no_view_p3_c3": (cs.oracle_mesh("2x2x2", 1), 3, 3, []),
    }


def names():
    return sorted(cases())


def write(path, mesh, P, channels, views):
    """ints n_vert n_tri has_bgr P C n_views; the mesh: xyz, faces (uint32), grey, bgr; per view: ints W H vch has_zbuf n_won,
    float64 K[4] pose7 tol min_area2, the image as the device holds it (vch channels), the z-buffer (float32); then the oracle's
    atlas, view (int32), score (float64), uv (float64) and the int n_textured."""
    r = to.texture(mesh, P, channels, views)
    X, F = np.ascontiguousarray(mesh["vertices"], np.float64), np.ascontiguousarray(mesh["faces"]).astype(np.uint32)
    bgr = mesh.get("colour") is not None
    with open(path, "wb") as fh:
        fh.write(np.array([len(X), len(F), bgr, P, channels, len(views)], np.int32).tobytes())
        fh.write(X.tobytes() + F.tobytes() + np.ascontiguousarray(mesh["grey"], np.uint8).tobytes())
        if bgr:
            fh.write(np.ascontiguousarray(mesh["colour"], np.uint8).tobytes())
        for v, n_won in zip(views, r["n_won"]):
            img = np.asarray(v["image"], np.uint8)
            img = to.view_image(img, 1) if channels == 1 or img.ndim == 2 else img           # grey unless a colour view meets 3 channels
            h, w = img.shape[:2]
            z = v.get("zbuf")
            fh.write(np.array([w, h, img.shape[2], z is not None, n_won], np.int32).tobytes())
            fh.write(np.array(list(v["K"]) + list(v["pose"]) + [v.get("tol", 0.0), v.get("min_area2", 0.0)], np.float64).tobytes())
            fh.write(np.ascontiguousarray(img).tobytes() + (b"" if z is None else np.ascontiguousarray(z, np.float32).tobytes()))
        fh.write(r["atlas"].tobytes() + r["view"].tobytes() + r["score"].tobytes() + r["uv"].tobytes())
        fh.write(np.array([r["n_textured"]], np.int32).tobytes())
    print(os.path.basename(path), len(X), "vertices", len(F), "triangles, atlas", r["atlas"].shape, "won", r["n_won"], "textured", r["n_textured"])


def main(out):
    os.makedirs(out, exist_ok=True)
    for name, (mesh, P, channels, views) in cases().items():
        write(os.path.join(out, name + ".bin"), mesh, P, channels, views)


if __name__ == "__main__":
    main(sys.argv[1])
