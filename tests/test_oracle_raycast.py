"""The ray-casting contract on the numpy oracle alone, and what of the library can be checked without a
device: the ABI table, the NULL-handle errors, every class of ray on the GPU test shapes, the box-skipping march against the
full one, and the accuracy conditions on the analytic sphere and on the plane scene (the kernel bodies on the host:
tests/test_host_checks.py).  CPU only."""
import ctypes as C

import numpy as np
import pytest

import dense_oracle as do
import dense_scene as ds
import fusion_oracle as fo
import fusion_scene as fs
import raycast_oracle as ro
import raycast_scene as rs

NAMES = ("ekf_raycast_render", "ekf_raycast_render_view", "ekf_raycast_get", "ekf_raycast_get_profile")
_CACHE = {}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    g.build()
    return g.load_package()


def _cases():
    """Every exact case and the oracle's full march of it, computed once."""
    if "cases" not in _CACHE:
        cases = rs.cases()
        _CACHE["cases"] = {k: (c, ro.raycast(**_kw(c))) for k, c in cases.items()}
    return _CACHE["cases"]


def _kw(c):
    c = dict(c)
    c["pose7"] = c.pop("pose")
    return c


def test_header_prototypes_and_exports_agree(pkg):
    from ekf_monoslam_amd import capi, fusion
    lib = pkg.load_library()
    names = [n for n in pkg.declared_symbols() if n.startswith("ekf_raycast_")]
    assert sorted(names) == sorted(n for n in capi._PROTOS if n.startswith("ekf_raycast_")) == sorted(NAMES)
    for n in names:
        assert hasattr(lib, n), n
    assert len([n for n in pkg.declared_symbols() if n.startswith("ekf_fusion_")]) == 12 and lib.ekf_abi_version() == 6
    assert all(hasattr(pkg, n) for n in ("Render", "shade", "audit_recording"))
    assert all(hasattr(fusion.TsdfVolume, n) for n in ("raycast", "raycast_view", "get_raycast_profile"))


def test_null_handle_calls_need_no_device(pkg):
    lib = pkg.load_library()
    K, pose = np.array([30.0, 30.0, 14.0, 11.0]), np.array([0.0, 0, -4, 1, 0, 0, 0])
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    w, h = C.c_int(7), C.c_int(7)
    assert lib.ekf_raycast_render(None, 29, 23, P(K), P(pose), 2.0, 6.5, 0.125, 1) == 1
    assert lib.ekf_raycast_render_view(None, None, 0, 2.0, 6.5, 0.125, 1) == 1
    assert lib.ekf_raycast_get(None, None, None, None, C.byref(w), C.byref(h)) == 1 and (w.value, h.value) == (7, 7)
    assert lib.ekf_raycast_get_profile(None, None, None) == 1


def test_every_class_of_ray_occurs_in_the_gpu_shapes():
    got = {k: r["stats"] for k, (c, r) in _cases().items()}
    for k, s in got.items():
        print(k, s)
    for k in ("sphere_A_step0", "sphere_A_step1", "sphere_B_step0", "sphere_B_step1"):
        assert got[k]["hits"] > 0 and got[k]["broken"] > 0
    for k in ("sphere_A_step2", "sphere_B_step2"):
        assert got[k]["in_to_out"] > 0 and got[k]["first_inside"] > 0 and got[k]["hits"] > 0
    assert got["sphere_A_near4"]["first_inside"] > 0 and got["sphere_A_near4"]["hits"] == 0
    for n in (0, 1):
        a, b, c = (got["main_%d_min%d" % (n, mc)] for mc in rs.MAIN_COUNTS)
        assert a["samples"] == rs.MAIN_N and a["hits"] > b["hits"] > 0 == c["hits"]
        assert a["rejected"] > 0 and a["broken"] > 100
    assert got["sphere_away"]["hits"] == got["empty"]["hits"] == 0 and got["sphere_1x1"]["hits"] == 1
    # a ray without a hit leaves depth 0, normal 0, grey 0; a hit has a unit normal
    for k, (c, r) in _cases().items():
        miss = r["depth"] == 0
        assert not r["normal"][miss].any() and not r["grey"][miss].any() and (r["depth"] >= 0).all()
        if (~miss).any():
            assert np.abs(np.linalg.norm(r["normal"][~miss].astype(np.float64), axis=1) - 1.0).max() < 1e-6


def test_box_skipping_march_equals_the_full_march():
    skipped = 0
    for k, (c, full) in _cases().items():
        part = ro.raycast(skip_box=True, **_kw(c))
        assert all(part[n].tobytes() == full[n].tobytes() for n in ("depth", "normal", "grey")), k
        skipped += part["stats"]["skipped"]
    # directions with a zero component, a camera inside the box, and one outside it on an axis it never leaves
    vol = fs.sphere_volume()
    for pose, K in ((rs.POSE_A, (30.0, 30.0, 14.0, 11.0)), (np.array([0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]), (30.0, 30.0, 14.0, 11.0)),
                    (np.array([5.0, 0.0, -4.0, 1.0, 0.0, 0.0, 0.0]), (1e9, 30.0, 14.0, 11.0))):
        kw = dict(_kw(rs.sphere_case(pose, 0.125, z_near=0.0, vol=vol)), K=K)
        full, part = ro.raycast(**kw), ro.raycast(skip_box=True, **kw)
        assert all(part[n].tobytes() == full[n].tobytes() for n in ("depth", "normal", "grey"))
    print("samples skipped", skipped)
    assert skipped > 10000


def _sphere_truth(pose):
    """(in the silhouette, analytic depth, the rays) of the sphere view from `pose`: the nearer root of |t + z dw| = r."""
    t, dw = ro.rays(rs.SPHERE_SHAPE, rs.SPHERE_K, pose)
    dw = np.stack(dw, axis=1)
    a, b, c = (dw * dw).sum(axis=1), (dw @ t), t @ t - fs.SPHERE_RADIUS ** 2
    disc = b * b - a * c
    z = (-b - np.sqrt(np.maximum(disc, 0.0))) / a
    return disc >= 0.0, z, t, dw


def test_accuracy_condition_sphere():
    """At step 0.125 no pixel outside the analytic silhouette is hit; of the hit pixels at least 90 % lie within 0.5 voxel of
    the analytic depth and at least 90 % have a normal within 10 degrees of the radial direction at the rendered point (the
    oracle's shares: 100 % and 100 %; the worst depth 0.16 voxel at pose A and 0.43 at pose B, the worst angle 7.97 degrees)."""
    for name, pose in (("A", rs.POSE_A), ("B", rs.POSE_B)):
        r = _cases()["sphere_%s_step0" % name][1]
        inside, z, t, dw = _sphere_truth(pose)
        depth, normal = r["depth"].reshape(-1).astype(np.float64), r["normal"].reshape(-1, 3).astype(np.float64)
        hit = depth > 0
        err = np.abs(depth[hit] - z[hit]) / fs.SPHERE_VOXEL
        X = t + depth[hit, None] * dw[hit]
        cosang = (normal[hit] * X).sum(axis=1) / np.linalg.norm(X, axis=1)
        ang = np.degrees(np.arccos(np.clip(cosang, -1.0, 1.0)))
        share_d, share_n = float((err <= 0.5).mean()), float((ang <= 10.0).mean())
        print("pose", name, "hits", int(hit.sum()), "of", int(inside.sum()), "in the silhouette; within 0.5 voxel", share_d, "worst", err.max(),
              "voxel; within 10 degrees", share_n, "worst", ang.max())
        assert hit.sum() > 200 and not (hit & ~inside).any()
        assert share_d >= 0.90 and share_n >= 0.90


def test_accuracy_condition_plane():
    """The true depth maps of the plane scene fused as in §16.5 and rendered at their three poses with step voxel / 2: at
    least 90 % of the hit pixels lie within 0.1 voxel of the true depth (the oracle's share: 100 %, the worst 0.005 voxel;
    2727, 2511 and 2551 hits of 2867)."""
    maps = fs.accuracy_maps()
    vol = fo.empty_volume(fs.ACC_DIMS)
    for m in maps:
        fo.integrate(vol, fs.ACC_DIMS, fs.ACC_ORIGIN, fs.ACC_VOXEL, fs.ACC_TRUNC, *m)
    for s, (z, img, K, pose) in zip(fs.ACC_SLOTS, maps):
        r = ro.raycast(vol, fs.ACC_DIMS, fs.ACC_ORIGIN, fs.ACC_VOXEL, (ds.W, ds.H), K, pose, float(z.min()) - fs.ACC_TRUNC,
                       float(z.max()) + fs.ACC_TRUNC, fs.ACC_VOXEL / 2.0, 1)
        hit = r["depth"] > 0
        err = np.abs(r["depth"][hit].astype(np.float64) - z[hit].astype(np.float64)) / fs.ACC_VOXEL
        share = float((err <= 0.1).mean())
        print("slot", s, "hits", int(hit.sum()), "of", hit.size, "share within 0.1 voxel", share, "worst", err.max(), "voxel",
              "mean |grey - image|", np.abs(r["grey"][hit].astype(float) - img[hit]).mean())
        assert hit.sum() >= 1000 and share >= 0.90


def test_shade_of_the_binding_equals_the_oracle(pkg):
    r = _cases()["sphere_B_step0"][1]
    for light in ((0.0, 0.0, -1.0), (1.0, -2.0, -2.0)):
        got = pkg.shade(pkg.Render(r["depth"], r["normal"], r["grey"]), light)
        assert got.dtype == np.uint8 and np.array_equal(got, ro.shade(r["normal"], r["depth"], light))
    img = pkg.shade(pkg.Render(r["depth"], r["normal"], r["grey"]))
    assert img[r["depth"] == 0].max() == 0 and img.max() > 200
