"""The mirror rule of the bf16x6 covariance downdate (EKF_SYRK_MIRROR_SKIP).

Launches 0 .. G-2 of an update store a strictly lower tile's mirror only where the re-evaluation of the next chunk's W
columns reads it; the last launch stores every mirror.  The rule moves stores, never arithmetic: mu and the FULL Sigma of
three predict + update frames equal the run with the knob at 0 (every launch mirrors every tile) to the last bit, Sigma is
exactly symmetric, and the launch counter of the launches that ran with bounds proves that the knob acted.

N = 640 (n = 3854: 31 tile rows, the bf16x6 path; m = 1280: more than one column chunk), the size of
test_launch_structure_knobs_are_bit_identical."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_FEAT = 640
FRAMES = 3
S_LIN = 2.0 ** -14          # scale of the inverse-depth row / column that sends a feature through the linearity test


def _stream():
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    px0, z = synthetic.measurement_stream(cfg, N_FEAT, FRAMES, sigma_px=0.5)
    return pkg, cfg, px0, z


def _subset():
    """600 of the 640 features drawn at random (the API takes a measured list in ascending order only -- ekf_update returns
    EKF_ERR_ARG for any other -- so the draw is sorted): irregular gaps, so no workgroup of the W kernel sees a run of
    neighbours, and bounds that span almost the whole state."""
    rng = np.random.default_rng(7)
    return np.sort(rng.permutation(N_FEAT)[:600]).astype(np.int32)


def _run(case, pkg, cfg, px0, z):
    kw = {"camera_dim": 13} if case == "camera13" else {}
    f = pkg.VSlamFilter(cfg, capacity_features=N_FEAT, **kw)
    f.setDt(1.0 / 30.0)
    for (u, v) in px0:
        assert f.addFeature((u, v)) == 1
    idx = _subset() if case == "subset_plane" else np.arange(N_FEAT, dtype=np.int32)
    plane = case == "subset_plane"
    nxyz = 0
    for k in range(FRAMES):
        f.predict()
        f.update(z[k][idx].reshape(-1), idx, plane_constraint=plane)
        if k == 0 and case == "xyz":
            # as test_remove_and_convert: a tiny inverse-depth variance sends a feature through the linearity test (here as
            # a congruence D Sigma D with an exact power of two, so Sigma stays symmetric and positive)
            pos, _ = f.featureLayout()
            S = f.getFullSigma()
            for i in range(5, N_FEAT, 9):
                S[pos[i] + 5, :] *= S_LIN
                S[:, pos[i] + 5] *= S_LIN
            f.setSigmaBlock(S)
            nxyz = f.convert2XYZ_ifLinearAll()
        if k == 0 and case == "lifecycle":
            # 1 % of the features leave, as many arrive (unmeasured, at the end of the state): the life-cycle kernels read
            # rows AND columns of Sigma, so a stale upper element would show in what they leave behind
            gone = np.arange(50, N_FEAT, 100, dtype=np.int32)[:6]
            f.removeFeatures(gone)
            for i in gone:
                assert f.addFeature(px0[i]) == 1
            keep = np.setdiff1d(np.arange(N_FEAT), gone)
            z = z[:, keep]
            idx = np.arange(keep.size, dtype=np.int32)
    f.synchronize()
    out = (f.getFullState(), f.getFullSigma(), f.chunkPlan(), f.launch_counts(), f.checkInvariants(), nxyz)
    f.close()
    return out


@pytest.mark.parametrize("case", ["all_ascending", "subset_plane", "camera13", "xyz", "no_w_recompute", "lifecycle"])
def test_mirror_skip_is_bit_identical(monkeypatch, case):
    """Per case: knob at its default against EKF_SYRK_MIRROR_SKIP=0.
    all_ascending   every feature measured, in ascending order (the fast path of the W kernel, tight bounds)
    subset_plane    600 features drawn at random + the plane rows (the W kernel's element-wise path, wide bounds, a last chunk
                    that holds the plane slots)
    camera13        the 13-wide camera layout of test_camera_dim_13_at_a_chunked_size: feature rows are not 16-byte aligned,
                    the front pad of the staged segment is 1 or 3
    xyz             some features converted to XYZ after the first frame (3-row features in the bounds)
    no_w_recompute  EKF_W_RECOMPUTE=0: nothing reads Sigma between the launches, the intermediate ones mirror nothing
    lifecycle       an update, then six features removed and six added, then two more updates"""
    pkg, cfg, px0, z = _stream()
    outs = []
    for knob in (None, "0"):
        monkeypatch.delenv("EKF_SYRK_MIRROR_SKIP", raising=False)
        monkeypatch.delenv("EKF_W_RECOMPUTE", raising=False)
        if knob is not None:
            monkeypatch.setenv("EKF_SYRK_MIRROR_SKIP", knob)           # read when the filter is created
        if case == "no_w_recompute":
            monkeypatch.setenv("EKF_W_RECOMPUTE", "0")
        outs.append(_run(case, pkg, cfg, px0, z))
    monkeypatch.delenv("EKF_SYRK_MIRROR_SKIP", raising=False)
    monkeypatch.delenv("EKF_W_RECOMPUTE", raising=False)
    (mu_a, S_a, plan_a, cnt_a, inv_a, nxyz_a), (mu_b, S_b, plan_b, cnt_b, inv_b, nxyz_b) = outs
    print(case, "chunk plan", plan_a, "bf16x6 launches", cnt_a["downdate_bf16x6"], "with bounds", cnt_a["downdate_mirror_bounds"],
          "/", cnt_b["downdate_mirror_bounds"], "xyz", nxyz_a)
    assert len(plan_a[1]) >= 2 and plan_a == plan_b
    assert plan_a[2] == (case != "no_w_recompute")
    # the knob acted: every bf16x6 launch of an update but the last ran with bounds, none with the knob at 0
    nchunks = len(plan_a[1])
    assert cnt_a["downdate_bf16x6"] == FRAMES * nchunks == cnt_b["downdate_bf16x6"]
    assert cnt_a["downdate_mirror_bounds"] == FRAMES * (nchunks - 1) and cnt_b["downdate_mirror_bounds"] == 0
    if case == "xyz":
        assert nxyz_a == nxyz_b and nxyz_a > 0
    assert np.all(np.isfinite(mu_a)) and np.all(np.isfinite(S_a))
    assert np.array_equal(mu_a, mu_b)
    assert np.array_equal(S_a, S_b)
    assert np.array_equal(S_a, S_a.T)
    for pad, asym, big in (inv_a, inv_b):
        assert pad == 0.0 and asym == 0.0, (pad, asym, big)
