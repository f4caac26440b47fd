"""The overlapped solves wait for the chain inside the kernel (EKF_SOLVE_POLL_CHAIN).

The solve of an overlapped chunk g >= 1 is launched on the second stream without a stream wait for the chain's event; its
workgroups poll the epoch word the chain's stream publishes for chunk g, then acquire.  The knob moves a wait, never
arithmetic: mu and the FULL Sigma of three predict + update frames equal the run with the knob at 0 (every overlapped solve
behind hipStreamWaitEvent) to the last bit, Sigma is exactly symmetric, the invariants and the status are clean (a poll that
gave up raises the status and getFullState fails), and the launch counter of the polling solves proves that the knob acted.

N = 640 (n = 3854: 31 tile rows, the bf16x6 path; m = 1280: three column chunks, so chunk 1 polls), the size and the cases
of tests/test_downdate_mirror.py, plus the same update through update_device with resident z and indices."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_FEAT = 640
FRAMES = 3
S_LIN = 2.0 ** -14          # scale of the inverse-depth row / column that sends a feature through the linearity test
KNOB = "EKF_SOLVE_POLL_CHAIN"


def _stream():
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    px0, z = synthetic.measurement_stream(cfg, N_FEAT, FRAMES, sigma_px=0.5)
    return pkg, cfg, px0, z


def _subset():
    """600 of the 640 features drawn at random, sorted (the API takes ascending lists only): the element-wise path of the W
    kernel, and a last chunk that holds the plane slots."""
    rng = np.random.default_rng(7)
    return np.sort(rng.permutation(N_FEAT)[:600]).astype(np.int32)


def _run(case, pkg, cfg, px0, z):
    import torch
    kw = {"camera_dim": 13} if case == "camera13" else {}
    f = pkg.VSlamFilter(cfg, capacity_features=N_FEAT, **kw)
    f.setDt(1.0 / 30.0)
    for (u, v) in px0:
        assert f.addFeature((u, v)) == 1
    idx = _subset() if case == "subset_plane" else np.arange(N_FEAT, dtype=np.int32)
    plane = case == "subset_plane"
    nxyz = 0
    keep_alive = []
    for k in range(FRAMES):
        f.predict()
        if case == "device_list":
            d_z = torch.from_numpy(np.ascontiguousarray(z[k][idx].reshape(-1), np.float32)).cuda()
            d_i = torch.from_numpy(idx).cuda()
            keep_alive += [d_z, d_i]                     # resident inputs must outlive the step
            f.update_device(d_z.data_ptr(), d_i.data_ptr(), idx.size)
        else:
            f.update(z[k][idx].reshape(-1), idx, plane_constraint=plane)
        if k == 0 and case == "xyz":
            pos, _ = f.featureLayout()
            S = f.getFullSigma()
            for i in range(5, N_FEAT, 9):
                S[pos[i] + 5, :] *= S_LIN
                S[:, pos[i] + 5] *= S_LIN
            f.setSigmaBlock(S)
            nxyz = f.convert2XYZ_ifLinearAll()
        if k == 0 and case == "lifecycle":
            gone = np.arange(50, N_FEAT, 100, dtype=np.int32)[:6]
            f.removeFeatures(gone)
            for i in gone:
                assert f.addFeature(px0[i]) == 1
            keep = np.setdiff1d(np.arange(N_FEAT), gone)
            z = z[:, keep]
            idx = np.arange(keep.size, dtype=np.int32)
    f.synchronize()                                      # (a status raised by a bounded wait fails here)
    out = (f.getFullState(), f.getFullSigma(), f.chunkPlan(), f.launch_counts(), f.checkInvariants(), nxyz)
    f.close()
    return out


@pytest.mark.parametrize("case", ["all_ascending", "subset_plane", "camera13", "xyz", "lifecycle", "device_list",
                                  "no_w_recompute"])
def test_solve_poll_chain_is_bit_identical(monkeypatch, case):
    """Per case: knob at its default against EKF_SOLVE_POLL_CHAIN=0 (the cases of test_mirror_skip_is_bit_identical;
    device_list: update_device with resident z and indices; no_w_recompute: EKF_W_RECOMPUTE=0, where the polling solve sits
    behind the right-looking W update instead of the re-evaluation)."""
    pkg, cfg, px0, z = _stream()
    outs = []
    for knob in (None, "0"):
        monkeypatch.delenv(KNOB, raising=False)
        monkeypatch.delenv("EKF_W_RECOMPUTE", raising=False)
        if knob is not None:
            monkeypatch.setenv(KNOB, knob)               # read when the filter is created
        if case == "no_w_recompute":
            monkeypatch.setenv("EKF_W_RECOMPUTE", "0")
        outs.append(_run(case, pkg, cfg, px0, z))
    monkeypatch.delenv(KNOB, raising=False)
    monkeypatch.delenv("EKF_W_RECOMPUTE", raising=False)
    (mu_a, S_a, plan_a, cnt_a, inv_a, nxyz_a), (mu_b, S_b, plan_b, cnt_b, inv_b, nxyz_b) = outs
    nchunks = len(plan_a[1])
    print(case, "chunk plan", plan_a, "polling solves", cnt_a["solve_poll_chain"], "/", cnt_b["solve_poll_chain"],
          "solves", cnt_a["solve"] + cnt_a["solve_two_groups"], "xyz", nxyz_a)
    assert nchunks >= 3 and plan_a == plan_b             # chunk 0 and the last chunk keep their stream waits
    # the knob acted: the solves of the overlapped chunks 1 .. G-2 of every update polled, none with the knob at 0
    assert cnt_a["solve_poll_chain"] == FRAMES * (nchunks - 2) and cnt_b["solve_poll_chain"] == 0
    for kind in ("solve", "solve_two_groups", "downdate_bf16x6", "w_recompute", "chain_step_launches", "chain_trail_diag"):
        assert cnt_a[kind] == cnt_b[kind], kind
    assert cnt_a["downdate_bf16x6"] == FRAMES * nchunks
    if case == "xyz":
        assert nxyz_a == nxyz_b and nxyz_a > 0
    assert np.all(np.isfinite(mu_a)) and np.all(np.isfinite(S_a))
    assert np.array_equal(mu_a, mu_b)
    assert np.array_equal(S_a, S_b)
    assert np.array_equal(S_a, S_a.T)
    for pad, asym, big in (inv_a, inv_b):
        assert pad == 0.0 and asym == 0.0, (pad, asym, big)
