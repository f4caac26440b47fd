"""Ray casting of the TSDF volume on the device against tests/raycast_oracle.py, bit for bit: the analytic
sphere from two poses at three steps and the integrated 19 x 13 x 11 volume at three values of min_count, through set_volume
and through real integration; a 1 x 1 view; a camera that looks away; repeated renders; the cache of the mean plane; a view
taken from a dense slot; the mesh of the last extract left alone; the state after the volume changed; every argument error
with the earlier render still readable; a living filter left untouched; and audit_recording end to end."""
import ctypes as C

import numpy as np
import pytest
import torch  # noqa: F401  (before the library is first loaded, as in test_gpu_fusion.py: one HIP runtime for both)

import fusion_oracle as fo
import fusion_scene as fs
import raycast_oracle as ro
import raycast_scene as rs

pytestmark = pytest.mark.gpu

_CACHE = {}


@pytest.fixture(scope="module")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


def _cases():
    """Every exact case with the oracle's render, computed once."""
    if "cases" not in _CACHE:
        out = {}
        for k, c in rs.cases().items():
            kw = dict(c)
            kw["pose7"] = kw.pop("pose")
            out[k] = (c, ro.raycast(**kw))
        _CACHE["cases"] = out
    return _CACHE["cases"]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(render, want):
    """Equal bit for bit."""
    return (render.depth.shape == want["depth"].shape and np.array_equal(_bits(render.depth), _bits(want["depth"])) and
            np.array_equal(_bits(render.normal), _bits(want["normal"])) and np.array_equal(render.grey, want["grey"]))


def _bytes(render):
    return render.depth.tobytes() + render.normal.tobytes() + render.grey.tobytes()


def _cast(v, c):
    return v.raycast(c["shape"], c["K"], c["pose"], c["z_near"], c["z_far"], c["step"], c["min_count"])


def _sphere(pkg):
    v = pkg.TsdfVolume(fs.SPHERE_DIMS, fs.SPHERE_ORIGIN, fs.SPHERE_VOXEL, fs.SPHERE_TRUNC)
    v.set_volume(*fs.sphere_volume())
    return v


def _main(pkg, integrate=True):
    v = pkg.TsdfVolume(fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC)
    if integrate:
        for m in fs.synthetic_maps():
            v.integrate_host(*m)
    else:
        v.set_volume(*fs.fused()[0][-1])
    return v


def test_sphere_renders_equal_the_oracle(pkg):
    v = _sphere(pkg)
    for k, (c, want) in _cases().items():
        if not k.startswith("sphere"):
            continue
        got = _cast(v, c)
        print(k, "hits", int((got.depth > 0).sum()), "oracle", want["stats"]["hits"], "differing depths",
              int((_bits(got.depth) != _bits(want["depth"])).sum()), "normals", int((_bits(got.normal) != _bits(want["normal"])).sum()),
              "greys", int((got.grey != want["grey"]).sum()))
        assert _same(got, want), k
    got = _cast(v, _cases()["sphere_away"][0])                       # the camera looks away: nothing but zeros
    assert not got.depth.any() and not got.normal.any() and not got.grey.any()
    one = _cast(v, _cases()["sphere_1x1"][0])
    assert one.depth.shape == (1, 1) and one.depth[0, 0] > 0
    # step None is voxel / 2
    c, want = _cases()["sphere_B_step0"]
    assert c["step"] == fs.SPHERE_VOXEL / 2 and _same(v.raycast(c["shape"], c["K"], c["pose"], c["z_near"], c["z_far"]), want)
    v.close()


@pytest.mark.parametrize("integrate", [True, False])
def test_main_volume_renders_equal_the_oracle(pkg, integrate):
    v = _main(pkg, integrate)
    for k, (c, want) in _cases().items():
        if not k.startswith("main"):
            continue
        got = _cast(v, c)
        print(k, "hits", int((got.depth > 0).sum()), "oracle", want["stats"]["hits"], "differing depths",
              int((_bits(got.depth) != _bits(want["depth"])).sum()), "normals", int((_bits(got.normal) != _bits(want["normal"])).sum()),
              "greys", int((got.grey != want["grey"]).sum()))
        assert _same(got, want), k
    v.reset()
    assert _same(_cast(v, _cases()["empty"][0]), _cases()["empty"][1])
    v.close()


def test_second_render_is_identical_and_the_mean_plane_cache_follows_min_count(pkg):
    v = _main(pkg)
    c = {mc: _cases()["main_0_min%d" % mc][0] for mc in (1, 2)}
    v.profile(True)
    first = _cast(v, c[1])
    again = _cast(v, c[1])
    assert _bytes(first) == _bytes(again)
    seq = [_cast(v, c[1]), _cast(v, c[2]), _cast(v, c[1])]
    prof = v.get_raycast_profile()
    print("profile", prof)
    assert prof["k_tsdf_raycast"][1] == 5 and prof["k_tsdf_mean"][1] == 3 and prof["k_tsdf_raycast"][0] > 0      # 1, (1), (1), 2, 1
    assert [v.get_profile()[k][1] for k in ("k_tsdf_integrate", "k_tsdf_count", "k_tsdf_scan", "k_tsdf_emit")] == [0, 0, 0, 0]
    v.profile(True)                                                 # a second profile(True) starts from zero
    assert set(v.get_raycast_profile().values()) == {(0.0, 0)}
    v.profile(False)
    assert _bytes(_cast(v, c[2])) == _bytes(seq[1])                 # switched off, launches leave the counts where they were
    assert set(v.get_raycast_profile().values()) == {(0.0, 0)} and set(v.get_profile().values()) == {(0.0, 0)}
    for got, mc in zip(seq, (1, 2, 1)):
        fresh = _main(pkg)
        assert _bytes(got) == _bytes(_cast(fresh, c[mc])) and _same(got, _cases()["main_0_min%d" % mc][1]), mc
        fresh.close()
    assert _bytes(seq[0]) != _bytes(seq[1])
    # an integration between two renders of one min_count: the plane is made again
    v.integrate_host(*fs.synthetic_maps()[0])
    vol = tuple(p.copy() for p in fs.fused()[0][-1])
    fo.integrate(vol, fs.DIMS, fs.ORIGIN, fs.VOXEL, fs.TRUNC, *fs.synthetic_maps()[0])
    kw = dict(c[1], vol=vol)
    kw["pose7"] = kw.pop("pose")
    assert _same(_cast(v, c[1]), ro.raycast(**kw))
    v.close()


def test_view_from_a_dense_slot_equals_raycast(pkg):
    depth, img, K, pose = fs.synthetic_maps()[1]
    d = pkg.DenseStereo(fs.MAP_W, fs.MAP_H, max_views=2)
    d.set_view(1, img, K, pose * np.array([1, 1, 1, 2, 2, 2, 2.0]))            # q is normalised by the slot
    v = _main(pkg)
    a = v.raycast_view(d, 1, rs.MAIN_NEAR, rs.MAIN_FAR, rs.MAIN_STEP, 1)
    _, K1, pose1 = d.view(1)
    b = v.raycast((fs.MAP_W, fs.MAP_H), K1, pose1, rs.MAIN_NEAR, rs.MAIN_FAR, rs.MAIN_STEP, 1)
    assert _bytes(a) == _bytes(b) and (a.depth > 0).sum() > 100
    lib = pkg.load_library()
    assert lib.ekf_raycast_render_view(v._h, d._h, 0, rs.MAIN_NEAR, rs.MAIN_FAR, rs.MAIN_STEP, 1) == 4       # an empty slot
    assert lib.ekf_raycast_render_view(v._h, d._h, 2, rs.MAIN_NEAR, rs.MAIN_FAR, rs.MAIN_STEP, 1) == 1
    assert lib.ekf_raycast_render_view(v._h, None, 0, rs.MAIN_NEAR, rs.MAIN_FAR, rs.MAIN_STEP, 1) == 1
    assert lib.ekf_raycast_render_view(v._h, d._h, 1, rs.MAIN_NEAR, rs.MAIN_FAR, 0.0, 1) == 1
    assert b"ekf_raycast_render_view" in lib.ekf_fusion_last_error(v._h)
    assert _bytes(v._render()) == _bytes(b)
    d.close()
    v.close()


def test_render_leaves_the_mesh_and_errors_leave_the_render(pkg):
    lib = pkg.load_library()
    P = lambda a: None if a is None else np.ascontiguousarray(a, np.float64).ctypes.data_as(C.c_void_p)
    v = _main(pkg)
    w, h = C.c_int(-1), C.c_int(-1)
    assert lib.ekf_raycast_get(v._h, None, None, None, C.byref(w), C.byref(h)) == 4 and (w.value, h.value) == (-1, -1)    # before a render
    mesh = v.extract(1)
    c, want = _cases()["main_1_min1"]
    got = _cast(v, c)
    assert _same(got, want)
    keep = pkg.Mesh(np.zeros_like(mesh.xyz), np.zeros_like(mesh.key), np.zeros_like(mesh.grey))
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.ekf_fusion_get_mesh(v._h, ptr(keep.xyz), ptr(keep.key), ptr(keep.grey), len(keep.xyz)) == 0
    assert all(getattr(keep, k).tobytes() == getattr(mesh, k).tobytes() for k in ("xyz", "key", "grey")) and len(mesh.xyz) > 0
    # an extract does not invalidate the render either
    v.extract(2)
    assert _bytes(v._render()) == _bytes(got)
    W, H = c["shape"]
    call = lambda width=W, height=H, K=c["K"], pose=c["pose"], z_near=c["z_near"], z_far=c["z_far"], step=c["step"], mc=1: \
        lib.ekf_raycast_render(v._h, width, height, P(K), P(pose), z_near, z_far, step, mc)
    nan, inf = np.nan, np.inf
    for bad in (dict(width=0), dict(height=0), dict(width=8193), dict(height=8193), dict(K=None), dict(pose=None),
                dict(K=[0.0, 24, 18, 9]), dict(K=[24.0, 0, 18, 9]), dict(K=[24.0, nan, 18, 9]), dict(K=[24.0, 24, inf, 9]),
                dict(pose=np.zeros(7)), dict(pose=[inf, 0, 0, 1, 0, 0, 0]), dict(step=0.0), dict(step=-0.05), dict(step=nan), dict(step=inf),
                dict(z_near=-0.01), dict(z_near=nan), dict(z_far=inf), dict(z_far=c["z_near"]), dict(z_near=1.0, z_far=0.5),
                dict(z_near=0.0, z_far=65536.5, step=1.0), dict(mc=0), dict(mc=65536)):
        assert call(**bad) == 1, bad
        assert b"ekf_raycast_render" in lib.ekf_fusion_last_error(v._h)
    assert call(K=[-24.0, 24, 18, 9]) == 0 and call(z_near=0.0, z_far=65535.5, step=1.0) == 0 and call() == 0     # the limits themselves
    assert lib.ekf_raycast_get_profile(v._h, None, None) == 1
    assert _bytes(v._render()) == _bytes(got)
    part = np.zeros((H, W), np.uint8)
    assert lib.ekf_raycast_get(v._h, None, None, ptr(part), None, None) == 0 and np.array_equal(part, want["grey"])
    # the volume changes: integrate, set_volume, reset
    v.integrate_host(*fs.synthetic_maps()[0])
    assert lib.ekf_raycast_get(v._h, None, None, None, C.byref(w), C.byref(h)) == 4
    with pytest.raises(pkg.EkfError) as ei:
        v._render()
    assert ei.value.status == 4
    _cast(v, c)
    v.set_volume(maps=-1)
    assert lib.ekf_raycast_get(v._h, None, None, None, None, None) == 4
    _cast(v, c)
    v.reset()
    assert lib.ekf_raycast_get(v._h, None, None, None, None, None) == 4
    v.close()


def test_a_living_filter_is_untouched(pkg):
    g = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=16, dtype=np.float32)
    for i in range(6):
        assert g.addFeature((40.0 + 50.0 * i, 60.0 + 30.0 * i)) == 1
    g.predict()
    g.synchronize()
    snap = lambda: (g.getFullState().tobytes(), g.getFullSigma().tobytes(), g.launch_counts())
    before = snap()
    v = _sphere(pkg)
    c, want = _cases()["sphere_A_step0"]
    assert _same(_cast(v, c), want)
    v.close()
    assert snap() == before
    g.close()


def test_audit_of_the_wall_recording_equals_the_oracles(pkg, tmp_path):
    """Five synthetic key frames of a textured wall -> audit_recording, against the oracles driven from the same files."""
    from ekf_monoslam_amd import dense, keyframes
    rec = str(tmp_path / "wall")
    ids = fs.write_wall_recording(rec, pkg.formats, keyframes.write_pgm)
    kw = dict(fs.REC_SWEEP)
    cost_trunc = kw.pop("trunc")
    got = pkg.audit_recording(rec, None, sweep_trunc=cost_trunc, **kw)
    kw["trunc_cost"] = cost_trunc
    z_near, z_far, step, frames = rs.oracle_audit_from_recording(dense.read_recording, dense.neighbours_of, rec, **kw)
    assert (got.z_near, got.z_far, got.step) == (z_near, z_far, step) and [f.id for f in got.frames] == ids
    assert len(got.mesh.faces) > 1000
    for f, want in zip(got.frames, frames):
        print("key frame", f.id, "overlap", f.overlap, "median", f.median, "p90", f.p90, "grey error", f.grey_error)
        assert _same(f.render, want["render"]), f.id
        assert (f.overlap, f.median, f.p90, f.grey_error) == (want["overlap"], want["median"], want["p90"], want["grey_error"])
    mid = got.frames[len(ids) // 2]
    assert mid.overlap > 0.3 and mid.median < 0.05                  # the wall seen again from where it was measured
    assert abs(float(np.median(mid.render.depth[mid.render.depth > 0])) - fs.REC_Z) < 0.05
