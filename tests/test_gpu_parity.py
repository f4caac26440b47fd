"""Parity of the HIP path (through the C ABI) with the CPU oracle on identical inputs.

Errors are rel-Frobenius.  Every comparison goes through helpers.bound(): the number written here is a CEILING per
class of comparison (fp32, one predict + update: Sigma 2e-5, mu 5e-6, Jacobians 4e-6, pixels 5e-4; fp64: 1e-10 /
1e-12), and tests/golden/parity_bounds.json tightens each call site to 10x the error MEASURED there on the MI355X
(profiles/r2_parity_measured.jsonl: e.g. 5e-7 .. 2e-6 on Sigma after one fp32 update, 1e-16 .. 2e-15 in fp64).
A failing assert prints the measured value."""
import os
import sys

import numpy as np
import pytest

import ekf_oracle as o
from helpers import bound, gpu_state, make_pair, oracle_cfg, relf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

TOL = {np.float64: dict(mu=1e-12, S=1e-10, h=1e-10, H=1e-10),
       np.float32: dict(mu=5e-6, S=2e-5, h=5e-4, H=4e-6)}


def step(ref, g, seed=1235, plane=False):
    ref.predict()
    g.predict()
    vis = ref.visible_indices()
    z = o.synthetic_measurements(ref, vis, seed=seed)
    ref.update(z, vis, plane=plane)
    g.update(z, vis, plane_constraint=plane)
    return vis, z


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_add_feature_matches_oracle(dtype):
    ref, g = make_pair(20, dtype, inject=False)
    mu, S = gpu_state(g)
    assert g.stateDim() == ref.n == 14 + 6 * 20
    pos, cod = g.featureLayout()
    assert list(pos) == [ft.position_in_state for ft in ref.features] and not cod.any()
    t = TOL[dtype]
    assert bound("mu, ref.mu", relf(mu, ref.mu), t["mu"] * 10)
    assert bound("S, ref.Sigma", relf(S, ref.Sigma), t["S"])
    assert g.addFeature((3.0, 100.0)) == 0            # outside the margin, vR.cpp:314


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("streaming", [0, 1])
def test_predict_matches_oracle(dtype, streaming):
    ref, g = make_pair(20, dtype)
    g.set_option(0, streaming)
    ref.predict([0.01, 0.0, -0.02], [0.0, 0.01, 0.0], True)
    g.predict([0.01, 0.0, -0.02], [0.0, 0.01, 0.0], True)
    mu, S = gpu_state(g)
    t = TOL[dtype]
    assert bound("mu, ref.mu", relf(mu, ref.mu), t["mu"])
    assert bound("S, ref.Sigma", relf(S, ref.Sigma), t["S"])
    h, vis, rem, S2, Hc, Hf = g.predictions(jacobians=True)
    assert list(np.nonzero(vis)[0]) == ref.visible_indices()
    assert not rem.any()
    Ft, Q = g.motionJacobian()                          # a2: System_model_jacobian + Q, compared directly
    assert bound("Ft, ref.Ft", relf(Ft, ref.Ft), t["H"]) and bound("Q, ref.Q", relf(Q, ref.Q), t["H"])
    for i, ft in enumerate(ref.features):
        assert bound("|h - ft.h| [px]", np.abs(h[i] - ft.h).max(), t["h"])
        assert bound("Hc[i], ft.Hc", relf(Hc[i], ft.Hc), t["H"])
        assert bound("Hf[i], ft.Hf", relf(Hf[i], ft.Hf), t["H"])
        k = ft.position_in_z
        assert bound("S2[i], ref.St[k:k + 2, k:k + 2]", relf(S2[i], ref.St[k:k + 2, k:k + 2]), t["S"] * 5)
    # second predict exercises the buffer flip of the streaming mode
    ref.predict()
    g.predict()
    mu, S = gpu_state(g)
    assert bound("S, ref.Sigma #2", relf(S, ref.Sigma), t["S"])


@pytest.mark.parametrize("dtype,mfma", [(np.float64, False), (np.float64, True), (np.float32, False), (np.float32, True)])
@pytest.mark.parametrize("n_feat", [20, 50])
def test_update_matches_oracle(dtype, mfma, n_feat):
    ref, g = make_pair(n_feat, dtype, mfma=mfma)
    vis, z = step(ref, g)
    g.synchronize()
    mu, S = gpu_state(g)
    t = TOL[dtype]
    assert bound("mu, ref.mu", relf(mu, ref.mu), t["mu"] * 5)
    assert bound("S, ref.Sigma", relf(S, ref.Sigma), t["S"])
    K = g.getGain()
    assert K.shape == ref.Kt.shape
    assert bound("K, ref.Kt", relf(K, ref.Kt), t["S"] * 20)
    assert abs(np.linalg.norm(mu[3:7]) - 1.0) < 1e-6


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_innovation_covariance_matches_oracle(dtype):
    ref, g = make_pair(20, dtype)
    ref.predict()
    g.predict()
    vis = ref.visible_indices()
    St = g.innovationCovariance(vis)
    assert bound("St, ref.St", relf(St, ref.St), TOL[dtype]["S"])
    sub = vis[3:11]
    assert bound("g.innovationCovariance(sub), ref.innovation_covariance(sub)", relf(g.innovationCovariance(sub), ref.innovation_covariance(sub)), TOL[dtype]["S"])
    assert bound("g.innovationCovariance(sub, True), ref.innovation_covariance(sub, True)", relf(g.innovationCovariance(sub, True), ref.innovation_covariance(sub, True)), TOL[dtype]["S"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dense_reference_formulation_agrees(dtype):
    """The faithful-dense oracle (the reference's own n^3 products) against the HIP path."""
    ref, g = make_pair(20, dtype, flavour=o.DenseFilter)
    step(ref, g)
    step(ref, g, seed=1236)
    mu, S = gpu_state(g)
    assert bound("mu, ref.mu", relf(mu, ref.mu), TOL[dtype]["mu"] * 10)
    assert bound("S, ref.Sigma", relf(S, ref.Sigma), TOL[dtype]["S"] * 2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_subset_and_plane_update(dtype):
    ref, g = make_pair(24, dtype)
    ref.predict()
    g.predict()
    vis = ref.visible_indices()[::2]
    z = o.synthetic_measurements(ref, vis)
    ref.update(z, vis, plane=True)
    g.update(z, vis, plane_constraint=True)
    mu, S = gpu_state(g)
    assert bound("mu, ref.mu", relf(mu, ref.mu), TOL[dtype]["mu"] * 5)
    assert bound("S, ref.Sigma", relf(S, ref.Sigma), TOL[dtype]["S"])


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_remove_and_convert(dtype):
    ref, g = make_pair(12, dtype)
    step(ref, g)
    # force two features through the linearity test on both sides
    for i in (2, 7):
        p = ref.features[i].position_in_state
        ref.Sigma[p + 5, p + 5] = 1e-9
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    assert ref.convert2xyz_if_linear_all() == 2
    assert g.convert2XYZ_ifLinearAll() == 2
    pos, cod = g.featureLayout()
    assert list(pos) == [ft.position_in_state for ft in ref.features]
    assert list(cod) == [ft.coding for ft in ref.features]
    mu, S = gpu_state(g)
    t = TOL[dtype]
    assert bound("mu, ref.mu", relf(mu, ref.mu), t["mu"] * 5) and bound("S, ref.Sigma", relf(S, ref.Sigma), t["S"])
    for i in (9, 4, 0):                              # descending, like vR.cpp:1296-1299
        ref.remove_feature(i)
    g.removeFeatures([0, 4, 9])
    assert g.numOfFeatures() == 9 and g.stateDim() == ref.n
    mu, S = gpu_state(g)
    assert bound("mu, ref.mu #2", relf(mu, ref.mu), t["mu"] * 5) and bound("S, ref.Sigma #2", relf(S, ref.Sigma), t["S"])
    xyz, cov = g.featureXYZ(1)                        # an XYZ feature after the shifts
    y_ref, c_ref = ref.feature_xyz(1)
    assert bound("xyz, y_ref", relf(xyz, y_ref), t["mu"] * 10) and bound("cov, c_ref", relf(cov, c_ref), t["S"] * 10)
    xyz, cov = g.featureXYZ(0)                        # inverse-depth feature: Jf Sigma Jf^T
    y_ref, c_ref = ref.feature_xyz(0)
    assert bound("xyz, y_ref #2", relf(xyz, y_ref), t["mu"] * 100) and bound("cov, c_ref #2", relf(cov, c_ref), t["S"] * 100)
    # mixed XYZ / inverse-depth map keeps working, and a new feature lands at the end
    assert g.addFeature((100.0, 90.0)) == 1 and ref.add_feature(100.0, 90.0) == 1
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    step(ref, g, seed=99)
    mu, S = gpu_state(g)
    pad, asym, big = g.checkInvariants()                # (the injected fp32 oracle Sigma is itself asymmetric at 1e-7)
    assert pad == 0.0 and asym <= 2e-6 * big, (pad, asym, big)
    assert bound("mu, ref.mu #3", relf(mu, ref.mu), t["mu"] * 10) and bound("S, ref.Sigma #3", relf(S, ref.Sigma), t["S"] * 2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_xyz_feature_jacobians_match_oracle(dtype):       # a5 (vR.cpp:552-578), compared directly
    ref, g = make_pair(12, dtype)
    step(ref, g)
    for i in (1, 5, 10):
        p = ref.features[i].position_in_state
        ref.Sigma[p + 5, p + 5] = 1e-9
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    assert ref.convert2xyz_if_linear_all() == 3 and g.convert2XYZ_ifLinearAll() == 3
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    ref.predict()
    g.predict()
    h, vis, rem, S2, Hc, Hf = g.predictions(jacobians=True)
    t = TOL[dtype]
    seen = 0
    for i, ft in enumerate(ref.features):
        assert bound("|h - ft.h| [px]", np.abs(h[i] - ft.h).max(), t["h"])
        assert bound("Hc[i], ft.Hc", relf(Hc[i], ft.Hc), t["H"])
        if ft.coding == o.XYZ:
            seen += 1
            assert ft.Hf.shape == (2, 3) and not Hf[i][:, 3:].any()          # 2x3 block, padding columns zero
            assert bound("Hf[i][:, :3], ft.Hf (XYZ)", relf(Hf[i][:, :3], ft.Hf), t["H"])
        else:
            assert bound("Hf[i], ft.Hf", relf(Hf[i], ft.Hf), t["H"])
        k = ft.position_in_z
        if ft.is_in_innovation:
            assert bound("S2[i], St block", relf(S2[i], ref.St[k:k + 2, k:k + 2]), t["S"] * 5)
    assert seen == 3
    assert list(np.nonzero(vis)[0]) == ref.visible_indices()


def test_getters_match_reference_semantics():
    ref, g = make_pair(8, np.float32)
    step(ref, g)
    assert g.getState().shape == (14,) and g.getSigma().shape == (14, 14)
    assert np.isclose(g.Covariance_Parameter(), float(ref.covariance_parameter()), rtol=1e-3)
    assert g.numOfFeatures() == 8 and np.isclose(g.getDt(), 1.0 / 30.0)
    blk = g.getSigmaBlock(14, 0, 6, 7)
    assert bound("blk, ref.Sigma[14:20, 0:7]", relf(blk, ref.Sigma[14:20, 0:7]), 1e-3)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_camera_dim_13(dtype):
    """(float32: through the fused predict and one-block update launches, whose row bookkeeping starts at camera_dim)"""
    ref, g = make_pair(10, dtype, camera_dim=13)
    step(ref, g)
    step(ref, g, seed=77)
    mu, S = gpu_state(g)
    assert g.stateDim() == 13 + 60
    assert bound("mu, ref.mu", relf(mu, ref.mu), TOL[dtype]["mu"] * 10)
    assert bound("S, ref.Sigma", relf(S, ref.Sigma), 1e-10 if dtype == np.float64 else TOL[dtype]["S"] * 2)


def test_camera_dim_13_at_a_chunked_size():
    """camera_dim = 13 (BASELINE's literal "13 + 6N") where the update is chunked (N = 640: ten block steps, three chunks):
    the feature columns then start at an odd multiple of 4 bytes past a 16-byte boundary, so the LDS-staged W kernel
    (k_sigma_ht_fast) must take its general path in EVERY workgroup -- in the first pass and in the re-evaluations of the
    sequential form.  Against the one-chunk path and the right-looking W update on the same inputs, two frames."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    n_feat = 640
    px0, z = synthetic.measurement_stream(cfg, n_feat, 2, sigma_px=0.5)
    idx = np.arange(n_feat, dtype=np.int32)
    outs = []
    for pipe, wrec in ((-1, 1), (-1, 0), (0, 1)):
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat, camera_dim=13)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        f.set_option(3, pipe)
        f.set_option(7, wrec)
        for k in range(2):
            f.predict()
            f.update(z[k].reshape(-1), idx)
        f.synchronize()
        assert f.stateDim() == 13 + 6 * n_feat
        pad, asym, big = f.checkInvariants()
        assert pad == 0.0 and asym == 0.0
        outs.append((f.getFullState(), f.getFullSigma(), f.chunkPlan()))
        f.close()
    (mu_a, S_a, plan_a), (mu_b, S_b, plan_b), (mu_c, S_c, plan_c) = outs
    assert len(plan_a[1]) == 3 and plan_a[2] and not plan_b[2] and len(plan_c[1]) == 1
    assert np.all(np.isfinite(mu_a)) and abs(np.linalg.norm(mu_a[3:7]) - 1.0) < 1e-6
    assert bound("mu: recompute vs right-looking", relf(mu_a, mu_b), 2e-5) and bound("Sigma: recompute vs right-looking", relf(S_a, S_b), 2e-4)
    assert bound("mu: chunked vs one chunk", relf(mu_a, mu_c), 2e-5) and bound("Sigma: chunked vs one chunk", relf(S_a, S_c), 2e-4)


def test_n200_stream_tracks_oracle():
    """configs[1] shape (N=200, fp32): 40 frames of the stream, free-running (no re-sync: injecting the
    oracle's slightly asymmetric Sigma into the symmetric HIP filter only adds error).  Measured on the
    MI355X: HIP-vs-fp32-oracle stays <= 1e-4 (Sigma) / 3e-6 (mu), and the HIP filter ends CLOSER to the
    fp64 oracle than the fp32 oracle does (it keeps Sigma symmetric and never forms (I-KH)Sigma)."""
    ref, g = make_pair(200, np.float32)
    ref64 = o.build_scenario(o.StructuredFilter, o.Config.kinect(), 200, np.float64)
    for k in range(40):
        ref.predict()
        g.predict()
        ref64.predict()
        vis = ref.visible_indices()
        z = o.synthetic_measurements(ref, vis, seed=2000 + k, sigma=0.5)
        ref.update(z, vis)
        g.update(z, vis)
        ref64.update(z.astype(np.float64), vis)
        mu, S = gpu_state(g)
        assert bound("mu, ref.mu", relf(mu, ref.mu), 2e-5), k
        assert bound("S, ref.Sigma", relf(S, ref.Sigma), 3e-4), k
    assert bound("mu, ref64.mu", relf(mu, ref64.mu), 2e-5) and bound("S, ref64.Sigma", relf(S, ref64.Sigma), 3e-4)
    assert bound("S, ref64.Sigma #2", relf(S, ref64.Sigma), 2.0 * relf(ref.Sigma, ref64.Sigma))


def test_n200_full_1000_frame_stream_with_resync():
    """BASELINE configs[1] as specified: N = 200 inverse-depth features, fp32, the 1000-frame synthetic measurement
    stream of the bench (static cloud, periodic camera trajectory, every visible feature measured in every frame).

    Per frame the HIP state is compared with the fp32 structured oracle running beside it; every K = 25 frames the
    ORACLE is re-synchronised to the HIP state (mu and the exactly symmetric Sigma are injected into it, never the other
    way round), so each comparison measures at most K frames of independent rounding (1000-frame streams
    diverge chaotically in fp32).  In every fifth segment (200 frames in all, the start-up segment included) an fp64
    oracle runs from the same start as well: it is the truth of that segment.  Measured on the MI355X
    (tools/stream_parity_probe.py, profiles/r2_stream_parity_probe.txt):
      * HIP vs fp64 oracle: 5e-6 .. 5e-5 on Sigma, 2e-7 .. 8e-7 on mu -- held to 10x that;
      * HIP vs fp32 oracle: 1e-4 .. 5e-4 on Sigma -- which is the fp32 ORACLE's rounding (explicit inverse and the
        (I - K H) Sigma form, vR.cpp:1276-1279), not the HIP path's: the fp32 oracle is as far from the fp64 one.  The test
        asserts exactly that where the fp64 truth runs: |HIP - o32| <= 1.5 |o32 - o64| + the HIP bound.
    A free-running fp64 oracle over the whole stream (own process, beside the loop) bounds the END state."""
    import multiprocessing as mp
    from threadpoolctl import threadpool_limits
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    import oracle_worker
    N, frames, K = 200, 1000, 25
    cfg = pkg.kinect_config()
    dT = 1.0 / 30.0
    px0, zs = synthetic.measurement_stream(cfg, N, frames, sigma_px=0.5)
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    worker = ctx.Process(target=oracle_worker.free_running_oracle, args=(px0, zs, "float64", dT, queue), daemon=True)
    worker.start()
    refs = {}
    for T in (np.float32, np.float64):
        r = o.StructuredFilter(o.Config.kinect(), T)
        r.dT = dT
        for (u, v) in px0:
            assert r.add_feature(u, v) == 1
        refs[T] = r
    ref, ref64 = refs[np.float32], refs[np.float64]
    g = pkg.VSlamFilter(cfg, capacity_features=N, dtype=np.float32)
    g.setDt(dT)
    for (u, v) in px0:
        assert g.addFeature((u, v)) == 1
    w = dict(mu64=0.0, S64=0.0, mu32=0.0, S32=0.0, h=0.0, excess=-1.0)
    # n = 1214 matrices: more BLAS threads than cores only slow the oracles down (the GPU box shows 64+ hardware
    # threads to numpy and grants 16 cores; the free-running oracle in the other process takes 4 of them)
    limiter = threadpool_limits(limits=8)
    truth = True                                            # is the fp64 oracle running in this segment?
    for k in range(frames):
        live = [ref, ref64] if truth else [ref]
        for r in live:
            oracle_worker.predict_no_St(r)
        g.predict()
        vis = ref.visible_indices()
        h, gvis, grem, _ = g.predictions()
        assert list(np.nonzero(gvis)[0]) == vis, k
        w["h"] = max(w["h"], float(np.abs(h - np.stack([ft.h for ft in ref.features])).max()))
        z = zs[k][vis].reshape(-1)
        for r in live:
            r.update(z.astype(r.T), vis)
        g.update(z, vis)
        mu, S = gpu_state(g)                               # synchronises: raises if a Cholesky pivot was not positive
        e_mu32, e_S32 = relf(mu, ref.mu), relf(S, ref.Sigma)
        assert e_mu32 < 1e-4 and e_S32 < 1e-2, (k, e_mu32, e_S32)   # hard stop per frame; the bounds are on the maxima
        w["mu32"], w["S32"] = max(w["mu32"], e_mu32), max(w["S32"], e_S32)
        if truth:
            e_mu64, e_S64 = relf(mu, ref64.mu), relf(S, ref64.Sigma)
            w["mu64"], w["S64"] = max(w["mu64"], e_mu64), max(w["S64"], e_S64)
            w["excess"] = max(w["excess"], e_S32 - 1.5 * relf(ref.Sigma, ref64.Sigma))
        if (k + 1) % K == 0:
            truth = ((k + 1) // K) % 5 == 0
            for r in ([ref, ref64] if truth else [ref]):
                r.mu, r.Sigma = mu.astype(r.T), S.astype(r.T)
    limiter.restore_original_limits()
    assert np.array_equal(S, S.T)                             # every kernel mirrors what it computes: exactly symmetric
    assert bound("per-frame mu vs fp64 oracle (every 5th segment), re-sync every 25", w["mu64"], 1e-5)
    assert bound("per-frame Sigma vs fp64 oracle (every 5th segment), re-sync every 25", w["S64"], 5e-4)
    assert bound("per-frame h [px] vs fp32 oracle", w["h"], 1e-3)
    assert bound("per-frame mu vs fp32 oracle, re-sync every 25", w["mu32"], 1e-5)
    assert bound("per-frame Sigma vs fp32 oracle, re-sync every 25 (the fp32 oracle's own rounding)", w["S32"], 3e-3)
    assert w["excess"] < 5e-4, w                             # |HIP - o32| - 1.5 |o32 - o64| on Sigma: explained by the oracle
    mu_end, S_end, partial = queue.get(timeout=300)
    worker.join(timeout=60)
    assert partial == 0
    assert bound("end mu vs free-running fp64 oracle (1000 frames)", relf(mu, mu_end), 1e-4)
    assert bound("end Sigma vs free-running fp64 oracle (1000 frames)", relf(S, S_end), 5e-3)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("seed,plane", [(0, False), (7, False), (12345, True), (99, False)])
def test_update_two_stage_composite_matches_oracle(dtype, seed, plane):
    """ekf_update_two_stage = the USE_RANSAC branch of VSlamFilter::update in one call (vR.cpp:964-1130 + 1245-1284):
    hypotheses, the reference's draw loop replayed from glibc's srand(seed) / rand() with the adaptive nhyp (:1030)
    (seed 0: best hypothesis), low-innovation update, rescue, second update with the plane rows."""
    ref, g = make_pair(30, dtype)
    ref.predict()
    g.predict()
    vis = ref.visible_indices()
    z = o.synthetic_measurements(ref, vis, sigma=1.0).reshape(-1, 2)
    z[4] += 7.0                                        # outside 2 sigma_px, maybe inside the chi2 gate
    z[13] += 60.0                                      # gross mismatches: never rescued
    z[21] -= 45.0
    # gate between the two kinds of outliers so that both outcomes of the rescue occur (the reference's gate of 1 is
    # very tight: S_hi carries no pixel noise)
    import copy
    probe = copy.deepcopy(ref)
    li0, _, _ = o.update_two_stage(probe, z, vis, plane=False, seed=seed)
    rest = [vis[k] for k in range(len(vis)) if not li0[k]]
    gate = 1.0
    if rest:
        _, chi2 = o.rescue_high_innovation(probe, ref.mu.copy(), z[~li0], rest, return_chi2=True)
        c = np.sort(np.asarray(chi2, np.float64))
        gate = float(np.sqrt(c[0] * c[-1])) if len(c) > 1 and c[0] > 0 else 1.0
    li_ref, hi_ref, drawn_ref = o.update_two_stage(ref, z, vis, plane=plane, seed=seed, chi2_threshold=gate)
    li, hi, drawn = g.updateTwoStage(z, vis, plane_constraint=plane, seed=seed, chi2_threshold=gate)
    assert drawn == drawn_ref and (seed == 0 or drawn < len(vis))          # the adaptive count stops the loop early
    assert list(li) == list(li_ref) and list(hi) == list(hi_ref)
    if seed == 0:                                      # (a replayed loop may end on an outlier's hypothesis: the reference's quirk, :1022)
        assert not li[13] and not li[21] and li.sum() >= len(vis) - 4
    mu, S = gpu_state(g)
    t = TOL[dtype]
    assert bound("mu, ref.mu", relf(mu, ref.mu), t["mu"] * 10) and bound("S, ref.Sigma", relf(S, ref.Sigma), t["S"] * 5)


def test_feature_noise_option_inflates_the_feature_variances_only():
    """EKF_OPT_FEATURE_NOISE (opt-in, off by default = the reference's static-map model): every predict adds
    v x 1e-12 to the variance of every feature state and leaves the camera block to the motion model."""
    ref, g = make_pair(12, np.float64)
    g.set_option(5, 2500000)                                  # 2.5e-6 per predict
    ref.predict()
    g.predict()
    d1 = np.diag(g.getFullSigma())
    dref = np.diag(ref.Sigma)
    assert np.allclose(d1[14:] - dref[14:], 2.5e-6, rtol=1e-6) and np.allclose(d1[:14], dref[:14], rtol=1e-12)


def test_fp32_covariance_stays_positive_over_a_long_all_measured_run():
    """Regression test of the downdate's rounding.  Sigma -= V V^T must accumulate V V^T on its own and meet Sigma
    once (one rounding at the magnitude of Sigma).  With the accumulators started at -Sigma -- every one of the 2M
    partial sums rounded at the magnitude of Sigma, products below half an ulp of it dropped -- the N = 400 map with
    every feature measured in every frame lost positivity near frame 900 and the Cholesky of S stopped at frame 1489
    (EKF_ERR_NUMERIC); the fp32 oracle in the reference's formulation stays positive to rounding, and so does this."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    N, frames = 400, 1800
    px0, zs = synthetic.measurement_stream(cfg, N, frames, sigma_px=0.5)
    idx = np.arange(N, dtype=np.int32)
    f = pkg.VSlamFilter(cfg, capacity_features=N)
    f.setDt(1.0 / 30.0)
    for (u, v) in px0:
        assert f.addFeature((u, v)) == 1
    for k in range(frames):
        f.predict()
        f.update(zs[k].reshape(-1), idx)                      # raises EkfError(EKF_ERR_NUMERIC) on a pivot <= 0
        if k % 100 == 99:
            f.synchronize()
    f.synchronize()
    P = f.getFullSigma().astype(np.float64)
    assert np.array_equal(P, P.T)
    w = np.linalg.eigvalsh(P)
    assert w[0] > -1e-9 * w[-1], (w[0], w[-1])                # positive to rounding (measured: -1e-12 .. -1e-17)


def test_error_paths():
    from __graft_entry__ import load_package
    pkg = load_package()
    ref, g = make_pair(4, np.float32, capacity=4)
    with pytest.raises(pkg.EkfError):                 # capacity
        g.addFeature((100.0, 100.0))
    with pytest.raises(pkg.EkfError):                 # update before predict
        g.update(np.zeros(2, np.float32), [0])
    g.predict()
    with pytest.raises(pkg.EkfError):
        g.update(np.zeros(2, np.float32), [7])
    with pytest.raises(pkg.EkfError):
        g.removeFeature(11)
    g.update()                                        # M = 0, no plane: no-op (vR.cpp:1266)


def test_nonpositive_rho_is_flagged_not_visible():     # vR.cpp:517-522
    ref, g = make_pair(6, np.float32)
    mu = ref.mu.copy()
    mu[ref.features[2].position_in_state + 5] = -0.05
    ref.mu = mu
    g.setFullState(mu)
    ref.measure()
    g.measure()
    h, vis, rem, S2, Hc, Hf = g.predictions(jacobians=True)
    assert rem[2] and not vis[2] and rem.sum() == 1
    assert ref.features[2].remove_flag and not ref.features[2].is_in_innovation
    assert bound("Hf[2], ref.features[2].Hf", relf(Hf[2], ref.features[2].Hf), 1e-3) and np.allclose(h[2], ref.features[2].h, atol=1e-2)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_search_ellipses_match_oracle(dtype):          # vR.cpp:1368-1382
    ref, g = make_pair(16, dtype)
    ref.predict()
    g.predict()
    ell = g.searchEllipses(sigma_size=4)
    for i, ft in enumerate(ref.features):
        k = ft.position_in_z
        a, b, th = o.ellipse_parameters(ref.St[k:k + 2, k:k + 2], 4)
        assert abs(int(ell[i, 0]) - a) <= 1 and abs(int(ell[i, 1]) - b) <= 1
        assert min(abs(int(ell[i, 2]) - th), 180 - abs(int(ell[i, 2]) - th)) <= 1
        assert ell[i, 0] <= ell[i, 1]


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_ransac_hypotheses_match_oracle(dtype):        # vR.cpp:986-1034
    ref, g = make_pair(24, dtype)
    ref.predict()
    g.predict()
    vis = ref.visible_indices()
    z = o.synthetic_measurements(ref, vis, sigma=1.0).reshape(-1, 2)
    z[3] += 40.0                                      # two gross mismatches
    z[11] -= 35.0
    counts_ref, mask_ref = o.ransac_1point(ref, z, vis)
    counts, best, inl = g.ransac1Point(z, vis)
    # borderline residuals (|e| within 1e-3 px of the threshold) may flip in fp32: allow one count
    assert np.abs(counts - counts_ref).max() <= (0 if dtype == np.float64 else 1)
    assert counts[best] == counts.max() and counts.max() >= len(vis) - 3
    assert not inl[3] and not inl[11]
    assert (inl != mask_ref[best]).sum() <= (0 if dtype == np.float64 else 1)
    # the usual two-stage use: update with the low-innovation inliers only
    sel = [vis[k] for k in range(len(vis)) if inl[k]]
    zz = z[inl].reshape(-1)
    ref.update(zz, sel)
    g.update(zz, sel)
    mu, S = gpu_state(g)
    assert bound("S, ref.Sigma", relf(S, ref.Sigma), TOL[dtype]["S"])


def test_plane_only_update_and_empty_map():
    """M = 0 with the forsePlane pseudo-measurement (vR.cpp:1250-1281), and a filter with no features."""
    ref, g = make_pair(6, np.float64)
    ref.predict()
    g.predict()
    ref.update(np.zeros(0), [], plane=True)
    g.update(np.zeros(0), [], plane_constraint=True)
    mu, S = gpu_state(g)
    assert bound("mu, ref.mu", relf(mu, ref.mu), 1e-11) and bound("S, ref.Sigma", relf(S, ref.Sigma), 1e-9)
    # remove everything, keep filtering on the 14-state camera
    g.removeFeatures(list(range(6)))
    for i in range(5, -1, -1):
        ref.remove_feature(i)
    assert g.numOfFeatures() == 0 and g.stateDim() == 14
    ref.predict()
    g.predict()
    g.update()
    ref.update(np.zeros(0), [], plane=True)
    g.update(np.zeros(0), [], plane_constraint=True)
    mu, S = gpu_state(g)
    assert bound("mu, ref.mu #2", relf(mu, ref.mu), 1e-11) and bound("S, ref.Sigma #2", relf(S, ref.Sigma), 1e-9)
    assert g.addFeature((120.0, 100.0)) == 1 and g.stateDim() == 20


def test_single_feature_update_f32():
    ref, g = make_pair(30, np.float32)
    ref.predict()
    g.predict()
    z = o.synthetic_measurements(ref, [17])
    ref.update(z, [17])
    g.update(z, [17])
    mu, S = gpu_state(g)
    assert bound("mu, ref.mu", relf(mu, ref.mu), 1e-5) and bound("S, ref.Sigma", relf(S, ref.Sigma), 2e-4)


def test_map_export_table():                         # RosVSLAMRansac.cpp:340-418
    ref, g = make_pair(10, np.float64)
    step(ref, g)
    for i in (1, 6):
        p = ref.features[i].position_in_state
        ref.Sigma[p + 5, p + 5] = 1e-9
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    assert ref.convert2xyz_if_linear_all() == 2 and g.convert2XYZ_ifLinearAll() == 2
    scale = float(ref.mu[13])
    pts = g.getPointsFeatures()
    allp = g.getPointsFeatures(convert_inverse_depth=True)
    for i, ft in enumerate(ref.features):
        y, C = ref.feature_xyz(i)
        if ft.coding == o.XYZ:
            assert np.allclose(pts[i, :3], y * scale, rtol=1e-10) and np.allclose(pts[i, 3:].reshape(3, 3), C, rtol=1e-9, atol=1e-15)
        else:
            assert not pts[i].any()                   # the reference leaves inverse-depth rows at zero
        assert np.allclose(allp[i, :3], y * scale, rtol=1e-9)
        assert np.allclose(allp[i, 3:].reshape(3, 3), C, rtol=1e-7, atol=1e-13)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_points_table_with_archived_patches(dtype):
    """The points.txt table in the reference's own layout (RosVSLAMRansac.cpp:340-418): rows by
    Patch::real_index, live XYZ rows, zero inverse-depth rows, and the XYZ + 3x3 covariance a removed feature leaves
    behind when it was found more than 5 times (deleted_patches, vR.cpp:394-404) -- captured on the device at the
    moment of removal -- against the oracle's restatement, through two-stage updates that drive n_find."""
    from ekf_monoslam_amd import formats
    ref, g = make_pair(14, dtype)
    f64 = dtype == np.float64
    for k in range(6):                                   # n_find: 1 -> 7 for the inliers of every frame
        ref.predict()
        g.predict()
        vis = ref.visible_indices()
        z = o.synthetic_measurements(ref, vis, seed=1235 + k, sigma=0.3)
        li, hi, _ = o.update_two_stage(ref, z, vis)
        li_g, hi_g, _ = g.updateTwoStage(z, vis)
        assert np.array_equal(li, li_g) and np.array_equal(hi, hi_g)
    ri, nf = g.featureIds()
    assert list(ri) == [ft.real_index for ft in ref.features] == list(range(1, 15))
    assert list(nf) == [ft.n_find for ft in ref.features] and max(nf) == 7
    for i in (1, 4, 6, 9):                               # make four features pass the linearity test: shrink rho's
        p = ref.features[i].position_in_state            # row AND column (a congruence: Sigma stays positive, the
        ref.Sigma[p + 5, :] *= 1e-4                      # updates that follow must still factorise S)
        ref.Sigma[:, p + 5] *= 1e-4
    g.setFullState(ref.mu)
    g.setSigmaBlock(ref.Sigma)
    assert ref.convert2xyz_if_linear_all() == 4 and g.convert2XYZ_ifLinearAll() == 4
    ref.features[9].n_find = 3                           # an XYZ feature that was NOT found often enough: not archived
    g.setFeatureMeta(9, n_find=3)
    # remove two XYZ features (one archived, one not), an inverse-depth one, and the LAST feature (the table shrinks
    # to the new last real_index); then add one: real_index continues at 15
    for i in (13, 9, 4, 2):
        ref.remove_feature(i)
    g.removeFeatures([2, 4, 9, 13])
    assert ref.add_feature(100.0, 90.0) == 1 and g.addFeature((100.0, 90.0)) == 1
    assert g.numArchived() == len(ref.deleted_patches) == 1
    step(ref, g)                                         # the live rows move on, the archived row must not
    want = o.get_points_features(ref)
    got = g.getPointsTable()
    assert got.shape == want.shape == (16, 12)
    assert not got[0].any() and not got[3].any()         # no patch 0; patch 3 (inverse depth, removed) left nothing
    assert got[5].any() and got[2].any() and got[7].any() and not got[10].any()
    assert bound("points table vs oracle", relf(got, want), 1e-9 if f64 else 2e-4)
    arch_real, arch_xyz, arch_cov = ref.deleted_patches[0]
    assert arch_real == 5 and np.allclose(got[5, 3:], arch_cov, rtol=1e-9 if f64 else 1e-4)
    text = formats.format_eigen(got)
    back = formats.read_points(__import__("io").StringIO(text))
    assert back.shape == got.shape and np.allclose(back, got, rtol=2e-5, atol=1e-30)


def test_full_size_properties_n1000():
    """BASELINE full size (N = M = 1000, n = 6014, fp32): size-independent properties instead of an
    oracle run -- Sigma stays symmetric and positive on its diagonal, every update shrinks the traced
    uncertainty of the measured features, the quaternion stays unit, streaming == in-place propagate,
    pipelined == serial update, and the innovation covariance factorises (no Cholesky failure)."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    N = 1000
    px0, z = synthetic.measurement_stream(cfg, N, 4, sigma_px=0.5)
    filters = []
    for opts in ({}, {0: 1}, {3: 0}):                 # default, streaming propagate, serial update
        f = pkg.VSlamFilter(cfg, capacity_features=N)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        for k, v in opts.items():
            f.set_option(k, v)
        filters.append(f)
    idx = np.arange(N, dtype=np.int32)
    d_prev = None
    for k in range(3):
        outs = []
        for f in filters:
            f.predict()
            if f is filters[0]:
                h, vis, rem, S2 = f.predictions()
                # (in the first frames a few inverse depths may dip below zero: the prior is rho0 = 0.2 +- 0.5)
                assert vis.sum() >= 0.98 * N and rem.sum() <= 0.02 * N
                assert np.all(S2[:, 0, 0] > 4.0) and np.all(S2[:, 1, 1] > 4.0)      # H Sigma H^T + 4 I
                d_pred = np.diag(f.getSigmaBlock(14, 14, 600, 600)).copy()
            f.update(z[k].reshape(-1), idx)
            f.synchronize()                           # raises if a Cholesky pivot was not positive
            outs.append((f.getFullState(), f.getSigmaBlock(0, 0, 620, 620)))
        mu, S = outs[0]
        assert np.all(np.isfinite(mu)) and abs(np.linalg.norm(mu[3:7]) - 1.0) < 1e-6
        assert np.abs(S - S.T).max() <= 1e-6 * np.abs(S).max()
        d = np.diag(S)
        assert np.all(d > 0)
        assert np.all(d[14:614] <= d_pred * (1 + 1e-5))       # a measurement never adds variance
        for mu2, S2_ in outs[1:]:
            assert bound("mu2, mu", relf(mu2, mu), 1e-5) and bound("S2_, S", relf(S2_, S), 1e-4)
    for f in filters:                                 # device-side invariants of the whole 6016 x 6016 buffer
        pad, asym, big = f.checkInvariants()
        assert pad == 0.0 and asym == 0.0 and big > 0.0, (pad, asym, big)
    full = filters[0].getFullSigma()
    assert full.shape == (6014, 6014) and np.array_equal(full, full.T)
    w = np.linalg.eigvalsh(full[:200, :200].astype(np.float64))
    assert w.min() > -1e-6 * w.max()                  # leading block stays positive semi-definite


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_two_stage_update_with_rescue(dtype):          # vR.cpp:964-1130, 1245-1284: the whole update() flow
    ref, g = make_pair(24, dtype)
    ref.predict()
    g.predict()
    vis = ref.visible_indices()
    z = o.synthetic_measurements(ref, vis, sigma=1.0).reshape(-1, 2)
    z[5] += 7.0                                        # outside 2 sigma_px of the prediction, inside the chi2 gate
    z[9] += 60.0                                       # a gross mismatch: never rescued
    counts, best, inl = g.ransac1Point(z, vis)
    counts_ref, mask_ref = o.ransac_1point(ref, z, vis)
    assert (inl != mask_ref[best]).sum() == 0 and not inl[5] and not inl[9]
    mu_before = ref.mu.copy()
    cam_before = g.getState()[:7]
    li = [vis[k] for k in range(len(vis)) if inl[k]]
    ref.update(z[inl].reshape(-1), li)
    g.update(z[inl].reshape(-1), li)
    rest = [vis[k] for k in range(len(vis)) if not inl[k]]
    hi1_ref, chi2 = o.rescue_high_innovation(ref, mu_before, z[~inl], rest, return_chi2=True)
    assert list(g.rescueHighInnovation(cam_before, z[~inl], rest)) == list(hi1_ref)     # the reference's gate (1)
    # the reference's gate is tight (S_hi carries no pixel noise); place it between the two outliers so
    # that both outcomes are exercised
    thr = float(np.sqrt(chi2[rest.index(vis[5])] * chi2[rest.index(vis[9])]))
    hi_ref = o.rescue_high_innovation(ref, mu_before, z[~inl], rest, threshold=thr)
    hi = g.rescueHighInnovation(cam_before, z[~inl], rest, thr)
    assert list(hi) == list(hi_ref)
    assert hi[rest.index(vis[5])] and not hi[rest.index(vis[9])]
    sel = [rest[k] for k in range(len(rest)) if hi[k]]
    zz = z[~inl][hi].reshape(-1)
    ref.update(zz, sel)
    g.update(zz, sel)
    mu, S = gpu_state(g)
    t = TOL[dtype]
    assert bound("mu, ref.mu", relf(mu, ref.mu), t["mu"] * 10) and bound("S, ref.Sigma", relf(S, ref.Sigma), t["S"] * 2)


@pytest.mark.parametrize("dtype,mfma,chunks", [(np.float64, False, 3), (np.float64, True, 3), (np.float32, True, 3), (np.float32, True, 2),
                                              (np.float32, False, 4)])
def test_chunked_pipeline_matches_oracle(dtype, mfma, chunks):
    """The chunked factorisation on two streams (what N = 1000 runs by default), forced on a map small
    enough for the oracle: diagonal-chunk inverses, right-looking W update, per-chunk downdates, and the
    gain by back-substitution over the chunks."""
    ref, g = make_pair(150, dtype, mfma=mfma)              # m = 300: 3 block steps (MFMA, 128) or 5 (64)
    g.set_option(3, chunks)                                # EKF_OPT_PIPELINE = k chunks
    vis, z = step(ref, g)
    g.synchronize()
    mu, S = gpu_state(g)
    t = TOL[dtype]
    assert bound("mu, ref.mu", relf(mu, ref.mu), t["mu"] * 5)
    assert bound("S, ref.Sigma", relf(S, ref.Sigma), t["S"] * 2)
    assert np.abs(S - S.T).max() <= 1e-6 * np.abs(S).max()
    K = g.getGain()
    assert K.shape == ref.Kt.shape and bound("K, ref.Kt", relf(K, ref.Kt), t["S"] * 50)
    # a second frame on the updated state, and agreement with the one-chunk path on the same inputs
    g1 = make_pair(150, dtype, mfma=mfma)[1]
    g1.set_option(3, 0)
    ref2, _ = make_pair(150, dtype, mfma=mfma)
    step(ref2, g1)
    mu1, S1 = gpu_state(g1)
    assert bound("mu1, mu", relf(mu1, mu), t["mu"] * 5) and bound("S1, S", relf(S1, S), t["S"])
    vis, z = step(ref, g, seed=77)
    mu, S = gpu_state(g)
    assert bound("mu, ref.mu #2", relf(mu, ref.mu), t["mu"] * 20) and bound("S, ref.Sigma #2", relf(S, ref.Sigma), t["S"] * 5)


@pytest.mark.parametrize("recompute", [1, 0])
def test_chunked_pipeline_with_subset_and_plane_rows_matches_oracle(recompute):
    """The sequential form of the chunked update (EKF_OPT_W_RECOMPUTE, round 4) where its special cases meet: a measured
    SUBSET (the runs of neighbouring features the LDS-staged W kernel looks for are broken: its per-workgroup fall-back),
    the three plane rows (columns of W that are columns of the downdated Sigma) and the identity padding behind them, three
    chunks forced on a map the oracle can follow -- against the fp32 oracle, with the right-looking W update (option 0)
    beside it on the same inputs."""
    ref, g = make_pair(210, np.float32)
    g.set_option(3, 3)                                     # three chunks (m = 2 * 170 + 3: three block steps of 128)
    g.set_option(7, recompute)
    ref.predict()
    g.predict()
    vis = ref.visible_indices()
    sel = [i for k, i in enumerate(vis) if k % 6 != 2][:170]      # gaps every sixth feature
    z = o.synthetic_measurements(ref, sel, seed=31)
    ref.update(z, sel, plane=True)
    g.update(z, sel, plane_constraint=True)
    g.synchronize()
    mu, S = gpu_state(g)
    t = TOL[np.float32]
    # measured on the MI355X: 2.0e-6 / 5.0e-6 (re-evaluated W), 2.6e-6 / 5.3e-6 (right-looking W update)
    assert bound("mu vs oracle", relf(mu, ref.mu), t["mu"] * 5)
    assert bound("Sigma vs oracle", relf(S, ref.Sigma), t["S"] * 2)
    assert np.array_equal(S, S.T)
    pad, asym, big = g.checkInvariants()
    assert pad == 0.0 and asym == 0.0
    block, ends, wrec = g.chunkPlan()
    assert block == 128 and ends == [1, 2, 3] and wrec == bool(recompute)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dynamic_resize_stream(dtype):
    """BASELINE configs[4] at oracle size: a measurement stream with features removed and added every few
    frames (vR.cpp:1296-1299 order: descending indices; additions land at the end), free-running on both
    sides -- the state dimension, the layout and every buffer the step sizes from n change under way."""
    ref, g = make_pair(60, dtype, capacity=80)
    rng = np.random.default_rng(1236)                       # add/delete schedule seed
    cfg = oracle_cfg()
    half = cfg.window_size // 2
    t = TOL[dtype]
    for frame in range(12):
        ref.predict()
        g.predict()
        vis = ref.visible_indices()
        z = o.synthetic_measurements(ref, vis, seed=2000 + frame, sigma=0.5)
        ref.update(z, vis)
        g.update(z, vis)
        if frame % 3 == 2:
            drop = sorted(rng.choice(len(ref.features), size=4, replace=False).tolist())
            for i in reversed(drop):
                ref.remove_feature(i)
            g.removeFeatures(drop)
            for _ in range(5):                               # one more than removed: the map also grows
                u = float(rng.uniform(half + 1, cfg.image_width - half - 1))
                v = float(rng.uniform(half + 1, cfg.image_height - half - 1))
                assert ref.add_feature(u, v) == 1 and g.addFeature((u, v)) == 1
            assert g.numOfFeatures() == len(ref.features) and g.stateDim() == ref.n
            pos, cod = g.featureLayout()
            assert list(pos) == [ft.position_in_state for ft in ref.features]
        mu, S = gpu_state(g)
        pad, asym, big = g.checkInvariants()                 # capacity 80 > N: the padding must stay exactly zero
        assert pad == 0.0 and asym <= 2e-6 * big, (frame, pad, asym, big)     # (the injected oracle Sigma is asymmetric at 1e-7)
        # free-running: rounding differences accumulate over the frames (fp32), none in fp64
        assert bound("mu, ref.mu", relf(mu, ref.mu), t["mu"] * (50 if dtype == np.float32 else 1e3)), frame
        assert bound("S, ref.Sigma", relf(S, ref.Sigma), t["S"] * (10 if dtype == np.float32 else 1e2)), frame
    assert g.numOfFeatures() == 64


@pytest.mark.parametrize("n_feat,m_meas,plane", [(700, 650, False), (530, 530, True)])
def test_mid_size_chunked_equals_serial(n_feat, m_meas, plane):
    """Sizes between the oracle's reach and the full benchmark, with a measured SUBSET and the plane rows:
    odd numbers of block steps (11 and 9), chunk ends that do not divide evenly -- default chunked two-stream
    update against the one-chunk path on identical inputs, two frames."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    px0, z = synthetic.measurement_stream(cfg, n_feat, 3, sigma_px=0.5)
    rng = np.random.default_rng(9)
    idx = np.sort(rng.choice(n_feat, size=m_meas, replace=False)).astype(np.int32)
    outs = []
    for pipe in (-1, 0):
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        f.set_option(3, pipe)
        for k in range(2):
            f.predict()
            f.update(z[k].reshape(-1, 2)[idx].reshape(-1), idx, plane)
        f.synchronize()
        outs.append((f.getFullState(), f.getFullSigma()))
    (mu_a, S_a), (mu_b, S_b) = outs
    assert np.all(np.isfinite(mu_a)) and abs(np.linalg.norm(mu_a[3:7]) - 1.0) < 1e-6
    # (the plane rows pull this camera far from its linearisation point: an ill-conditioned step that
    # amplifies fp32 rounding differences between the two schedules)
    tol = 2e-4 if plane else 1e-5
    assert bound("mu_a, mu_b", relf(mu_a, mu_b), tol) and bound("S_a, S_b", relf(S_a, S_b), 10 * tol)
    assert np.abs(S_a - S_a.T).max() <= 1e-6 * np.abs(S_a).max()


@pytest.mark.parametrize("wrec", ["0", "1"])
def test_fused_wupdate_launch_is_bit_identical(monkeypatch, wrec):
    """Exact-fp32 path (EKF_SPLIT_BF16 = 0; under the bf16x6 default EKF_FUSE_WU is not consulted): the right-looking update
    of a chunk -- all of W (EKF_W_RECOMPUTE = 0) or the innovation row only (= 1) -- riding in its downdate launch
    (EKF_FUSE_WU = 1: every overlapped chunk it pays for, 2: every overlapped chunk) runs the same tiles with the same
    per-tile arithmetic as separate launches (0): mu and Sigma agree to the last bit, and the launch counters show that
    the three modes really are three launch structures."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    n_feat = 640                                             # 10 block steps, chunks 2 / 4 / 10, 496 lower tiles >= 256 CUs
    px0, z = synthetic.measurement_stream(cfg, n_feat, 3, sigma_px=0.5)
    idx = np.arange(n_feat, dtype=np.int32)
    outs, counts = [], []
    monkeypatch.setenv("EKF_SPLIT_BF16", "0")
    monkeypatch.setenv("EKF_W_RECOMPUTE", wrec)
    for mode in ("0", "1", "2"):
        monkeypatch.setenv("EKF_FUSE_WU", mode)              # read when the filter is created
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        for k in range(2):
            f.predict()
            f.update(z[k].reshape(-1), idx)
        f.synchronize()
        outs.append((f.getFullState(), f.getFullSigma()))
        counts.append(f.launch_counts())
        f.close()
    for c in counts:
        assert c["downdate_bf16x6"] == 0, c
    assert counts[0]["downdate_f32_fused_wu"] == 0 and counts[0]["row_gemv" if wrec == "1" else "w_update_gemm"] >= 2, counts[0]
    assert counts[1]["downdate_f32_fused_wu"] >= 2, counts[1]
    assert counts[2]["downdate_f32_fused_wu"] >= counts[1]["downdate_f32_fused_wu"], (counts[1], counts[2])
    if wrec == "0":                                          # mode 1 leaves the chunk before the last to two launches, mode 2 fuses it too
        assert counts[2]["downdate_f32_fused_wu"] > counts[1]["downdate_f32_fused_wu"], (counts[1], counts[2])
    for mu, S in outs[1:]:
        assert np.array_equal(mu, outs[0][0]) and np.array_equal(S, outs[0][1])


def test_w_recompute_agrees_with_the_right_looking_w_update():
    """EKF_OPT_W_RECOMPUTE (default 1, round 4): the W columns of chunk g + 1 re-evaluated from the downdated Sigma
    (W' = Sigma' H^T: the sequential form of the update) against the right-looking GEMM update W -= V_g L^T of rounds 1-3
    (option 0) on identical inputs: the same update up to fp32 rounding, three frames, N = 640 (10 block steps, chunks
    3 / 5 / 10: two re-evaluations per frame) -- and both against the fp64 oracle's first frame at N = 1000 in
    test_n1000_default_pipeline_matches_fp64_oracle (default) / the sharded N = 1000 tests (right-looking)."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    n_feat = 640
    px0, z = synthetic.measurement_stream(cfg, n_feat, 3, sigma_px=0.5)
    idx = np.arange(n_feat, dtype=np.int32)
    outs = []
    for mode in (1, 0):
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        f.set_option(7, mode)
        for k in range(3):
            f.predict()
            f.update(z[k].reshape(-1), idx)
        f.synchronize()
        outs.append((f.getFullState(), f.getFullSigma(), f.checkInvariants()))
        f.close()
    (mu1, S1, inv1), (mu0, S0, inv0) = outs
    assert inv1[0] == 0.0 and inv1[1] == 0.0 and np.array_equal(S1, S1.T)
    assert not np.array_equal(S1, S0)                        # the re-evaluation path did run
    assert bound("mu: recompute vs right-looking", relf(mu1, mu0), 2e-5)
    assert bound("Sigma: recompute vs right-looking", relf(S1, S0), 2e-4)


@pytest.mark.parametrize("knobs,differs", [
    # exact-fp32 path (EKF_SPLIT_BF16 = 0): these knobs are only consulted there
    ({"EKF_SPLIT_BF16": "0", "EKF_SPLIT_TAIL": "0"}, ("downdate_f32_half_tail",)),      # no half tiles at the end of the last downdate's list
    ({"EKF_SPLIT_BF16": "0", "EKF_SPLIT_TAIL": "200"}, ()),                             # another number of half tiles (same launch kinds)
    ({"EKF_SPLIT_BF16": "0", "EKF_FUSE_WU": "0"}, ("downdate_f32_fused_wu", "row_gemv")),   # innovation-row update and downdate never in one launch
    ({"EKF_SPLIT_BF16": "0", "EKF_FUSE_WU": "0", "EKF_W_RECOMPUTE": "0"}, ("downdate_f32_fused_wu", "w_update_gemm")),
    ({"EKF_SPLIT_BF16": "0", "EKF_FUSE_WU": "2", "EKF_W_RECOMPUTE": "0"}, ("downdate_f32_fused_wu",)),
    ({"EKF_SPLIT_BF16": "0", "EKF_ROW_GEMV": "0", "EKF_FUSE_WU": "0"}, ("row_tile_gemm", "downdate_f32_fused_wu")),
    # bf16x6 path (the default): the knobs that act on it
    ({"EKF_ROW_GEMV": "0"}, ("row_rider", "row_tile_gemm")),                            # the innovation row through the tile GEMM: same bits by design
    ({"EKF_RESERVED_CUS": "24"}, ()), ({"EKF_RESERVED_CUS": "48"}, ()),                 # another grid for every overlapped launch, the same tiles
    ({"EKF_CHAIN_FUSED_DIAG": "0"}, ("chain_step_launches", "chain_trail_diag")),       # round 6: trailing update + next diagonal factor as one launch (default) against three launches per step
    ({"EKF_SPLIT_BF16": "0", "EKF_CHAIN_FUSED_DIAG": "0"}, ("chain_step_launches", "chain_trail_diag")),
    ({"EKF_TD_MIN_BLOCKS": "1"}, ("chain_trail_diag",)),
    ({"EKF_FUSE_SPLIT": "0"}, ("split_image",)),
    ({"EKF_SU_TAIL": "0"}, ("state_update_tail",)),                                     # round 6: mu += V y by the last downdate's idle workgroups against its own launch                                        # round 6: the plane image of V_g written by the solve's tiles against its own launch
    ({"EKF_CHAIN_DEFER": "0"}, ()),                                                     # a chunk's event behind / in front of its last trailing update: the same launches                                # ... for every step, however few blocks its update has
])
def test_launch_structure_knobs_are_bit_identical(monkeypatch, knobs, differs):
    """The tuning knobs of DESIGN.md section 3 change WHICH workgroup computes a tile, in which launch and in what tile
    shape, never the arithmetic of an element: mu and Sigma equal the reference configuration (the same arithmetic and W
    mode, every other knob at its default) to the last bit.  `differs`: the launch kinds whose counters must differ between
    the two runs -- the proof that the knob acted (under the bf16x6 default half of these knobs were
    dead and the test compared a configuration with itself)."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    n_feat = 640
    px0, z = synthetic.measurement_stream(cfg, n_feat, 3, sigma_px=0.5)
    idx = np.arange(n_feat, dtype=np.int32)
    outs, counts = [], []
    common = ("EKF_W_RECOMPUTE", "EKF_SPLIT_BF16")                       # arithmetic and W mode are common to both runs
    base = {k: v for k, v in knobs.items() if k in common}
    all_knobs = ("EKF_SPLIT_TAIL", "EKF_FUSE_WU", "EKF_W_RECOMPUTE", "EKF_SPLIT_BF16", "EKF_ROW_GEMV", "EKF_RESERVED_CUS",
                 "EKF_CHUNKS", "EKF_CHAIN_FUSED_DIAG", "EKF_TD_MIN_BLOCKS", "EKF_FUSE_SPLIT",
                 "EKF_CHAIN_DEFER", "EKF_SU_TAIL")
    for env in (base, knobs):
        for k in all_knobs:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)                             # read when the filter is created
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        for k in range(3):
            f.predict()
            f.update(z[k].reshape(-1), idx)
        f.synchronize()
        outs.append((f.getFullState(), f.getFullSigma()))
        counts.append(f.launch_counts())
        f.close()
    for k in all_knobs:
        monkeypatch.delenv(k, raising=False)
    split = knobs.get("EKF_SPLIT_BF16", "1") == "1"
    for c in counts:                                             # the arithmetic the parameter set names is the one that ran
        assert (c["downdate_bf16x6"] > 0) == split, c
        assert (c["downdate_f32"] + c["downdate_f32_fused_wu"] + c["downdate_f32_half_tail"] > 0) == (not split), c
    for kind in differs:
        assert counts[0][kind] != counts[1][kind], (kind, counts)
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("n_feat,stride,plane,nxyz,expect", [
    (8, 1, False, 0, True), (20, 1, True, 0, True), (32, 1, True, 0, True), (32, 2, False, 3, True),
    (21, 3, True, 1, True), (35, 1, True, 2, True), (35, 1, False, 0, True),
    (40, 1, True, 0, False),                               # n = 254, m = 83: the W image does not fit the LDS -> four launches
])
def test_small_map_onelaunch_update_is_bit_identical(monkeypatch, n_feat, stride, plane, nxyz, expect):
    """Round 6: the update of a small map (n_pad <= 256, the reference's 20-35 features) is ONE launch
    (k_update_small_onelaunch: every workgroup forms W, S and the factor for itself, then its own tile) instead of four.
    Every sum is formed by the instruction sequence of the kernel it replaces: mu, Sigma, the gain and the workspaces W
    and V (ekf_peek_workspace) equal the four-launch path (EKF_SMALL_ONELAUNCH=0) to the last bit -- all measured and
    subsets, with and without the plane rows, with XYZ features in the list -- and the launch counters prove which
    path ran."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    frames = 4
    px0, z = synthetic.measurement_stream(cfg, n_feat, frames, sigma_px=0.5)
    idx = np.arange(0, n_feat, stride, dtype=np.int32)
    outs, counts = [], []
    for mode in ("0", "1"):
        monkeypatch.setenv("EKF_SMALL_ONELAUNCH", mode)
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        per_frame = []
        for k in range(frames):
            if k == 1 and nxyz:
                pos, _ = f.featureLayout()
                nn = f.stateDim()
                for fi in range(1, 1 + 2 * nxyz, 2):          # force some features through the linearity test: a known depth
                    r = int(pos[fi]) + 5
                    f.setSigmaBlock(np.zeros((1, nn), np.float32), r, 0)
                    f.setSigmaBlock(np.zeros((nn, 1), np.float32), 0, r)
                    f.setSigmaBlock(np.array([[1e-9]], np.float32), r, r)
                assert f.convert2XYZ_ifLinearAll() == nxyz
            f.predict()
            f.update(z[k][idx].reshape(-1), idx, plane_constraint=plane)
            n = f.stateDim()
            npad = (n + 127) // 128 * 128
            per_frame.append((f.getFullState(), f.getFullSigma(), f.getGain(), f.peekWorkspace(0, 0, 0, npad + 1, 128),
                              f.peekWorkspace(1, 0, 0, npad + 1, 128)))
        assert f.checkInvariants()[0] == 0.0
        outs.append(per_frame)
        counts.append(f.launch_counts())
        f.close()
    monkeypatch.delenv("EKF_SMALL_ONELAUNCH", raising=False)
    assert counts[0]["update_onelaunch"] == 0 and counts[0]["update_allinone"] == frames, counts[0]
    if expect:
        assert counts[1]["update_onelaunch"] == frames and counts[1]["update_allinone"] == 0, counts[1]
    else:
        assert counts[1]["update_onelaunch"] == 0 and counts[1]["update_allinone"] == frames, counts[1]
    for k in range(frames):
        for name, a0, a1 in zip(("mu", "Sigma", "gain", "W", "V"), outs[0][k], outs[1][k]):
            assert np.array_equal(a0, a1), (k, name, float(np.max(np.abs(a0.astype(np.float64) - a1))))


@pytest.mark.parametrize("n_feat", [32, 200])
def test_update_device_equals_host_list_and_flags_bad_lists(n_feat):
    """`ekf_update_device` (z and the list resident on the device: what bench.py times) against `ekf_update` on the same inputs,
    bit for bit -- on the one-launch path of small maps (N = 32) and on the chunk path (N = 200) -- and the one check a resident
    list cannot get on the host: an index outside [0, N) or a list that is not strictly ascending raises the status word on the
    device (every kernel clamps what it reads meanwhile), and the next synchronising call returns EKF_ERR_ARG."""
    import torch
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    frames = 3
    px0, z = synthetic.measurement_stream(cfg, n_feat, frames, sigma_px=0.5)
    idx = np.arange(0, n_feat, 2, dtype=np.int32)
    d_idx = torch.from_numpy(idx).cuda()
    outs = []
    for resident in (False, True):
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        for k in range(frames):
            f.predict()
            zk = np.ascontiguousarray(z[k][idx].reshape(-1), np.float32)
            if resident:
                d_z = torch.from_numpy(zk).cuda()
                f.update_device(d_z.data_ptr(), d_idx.data_ptr(), len(idx), True)
                f.synchronize()
            else:
                f.update(zk, idx, plane_constraint=True)
        outs.append((f.getFullState(), f.getFullSigma()))
        if resident:
            for bad in (np.r_[idx[:-1], n_feat + 5].astype(np.int32), idx[::-1].copy()):
                f.predict()
                d_bad = torch.from_numpy(bad).cuda()
                d_z = torch.from_numpy(np.ascontiguousarray(z[0][idx].reshape(-1), np.float32)).cuda()
                with pytest.raises(pkg.EkfError) as e:
                    f.update_device(d_z.data_ptr(), d_bad.data_ptr(), len(bad), False)
                    f.synchronize()
                    f.getFullState()
                assert e.value.status == 1 and "device-resident index" in str(e.value), str(e.value)
        f.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("n_feat,stride,plane", [(70, 1, True), (200, 1, False), (200, 3, True), (230, 1, True)])
def test_fused_block_step_is_bit_identical(monkeypatch, n_feat, stride, plane):
    """Round 6: on maps whose chain is one column chunk (up to ~230 features: BASELINE configs[1]) a block step of the Cholesky
    chain -- diagonal factor, panel, trailing update -- is ONE launch (k_chain_step_fused: every tile workgroup factors the
    diagonal block and forms its two panel blocks for itself) instead of three.  Every sum is the sum of the launch it
    replaces: mu, Sigma and the gain equal the three-launch chain (EKF_STEP_FUSED=0) to the last bit; the launch counters
    prove which path ran (2 - 4 block steps per update here, measured subsets and plane rows included)."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    frames = 3
    px0, z = synthetic.measurement_stream(cfg, n_feat, frames, sigma_px=0.5)
    idx = np.arange(0, n_feat, stride, dtype=np.int32)
    outs, counts = [], []
    for mode in ("0", "1"):
        monkeypatch.setenv("EKF_STEP_FUSED", mode)
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        per = []
        for k in range(frames):
            f.predict()
            f.update(z[k][idx].reshape(-1), idx, plane_constraint=plane)
            per.append((f.getFullState(), f.getFullSigma(), f.getGain()))
        assert f.checkInvariants()[0] == 0.0
        outs.append(per)
        counts.append(f.launch_counts())
        f.close()
    monkeypatch.delenv("EKF_STEP_FUSED", raising=False)
    nblk = (2 * len(idx) + (3 if plane else 0) + 127) // 128
    assert nblk >= 2
    assert counts[0]["chain_step_fused"] == 0 and counts[1]["chain_step_fused"] == frames * nblk, (counts[0], counts[1])
    assert counts[1]["chain_step_launches"] == 0 and counts[0]["chain_step_launches"] > 0
    for k in range(frames):
        for name, a0, a1 in zip(("mu", "Sigma", "gain"), outs[0][k], outs[1][k]):
            assert np.array_equal(a0, a1), (k, name, float(np.max(np.abs(a0.astype(np.float64) - a1))))


def test_chunk_plan_knob_changes_rounding_only(monkeypatch):
    """EKF_CHUNKS (where the column chunks of the factorisation end) is NOT a bit-identity knob: another plan is another
    order of the sequential form (which columns of W are re-evaluated from which downdated Sigma).  Same update up to fp32
    rounding: N = 640 (10 block steps), three frames, the default plan 2 / 4 / 10 against 3 / 6 / 10 and against ONE chunk,
    on the default arithmetic."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    n_feat = 640
    px0, z = synthetic.measurement_stream(cfg, n_feat, 3, sigma_px=0.5)
    idx = np.arange(n_feat, dtype=np.int32)
    outs, plans = [], []
    for plan in (None, "3,6,10", "10"):
        monkeypatch.delenv("EKF_CHUNKS", raising=False)
        if plan:
            monkeypatch.setenv("EKF_CHUNKS", plan)
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        for k in range(3):
            f.predict()
            f.update(z[k].reshape(-1), idx)
        f.synchronize()
        outs.append((f.getFullState(), f.getFullSigma()))
        plans.append(f.chunkPlan()[1])
        assert f.launch_counts()["downdate_bf16x6"] == 3 * len(plans[-1])
        f.close()
    monkeypatch.delenv("EKF_CHUNKS", raising=False)
    assert plans[0] == [2, 4, 10] and plans[1] == [3, 6, 10] and plans[2] == [10], plans
    for k in (1, 2):
        assert not np.array_equal(outs[0][1], outs[k][1])
        assert bound(f"mu: plan {plans[k]} vs default", relf(outs[k][0], outs[0][0]), 2e-5)
        assert bound(f"Sigma: plan {plans[k]} vs default", relf(outs[k][1], outs[0][1]), 2e-4)
        assert np.array_equal(outs[k][1], outs[k][1].T)


def test_plain_step_repeats_bit_for_bit():
    """Work queues, two streams and persistent grids decide WHO computes a tile, never what it sums: two fresh filters fed the
    same calls (six frames at N = 1000, a removal of 1 % of the features and as many adds behind the third) end on the
    same bits, and the peeked workspace (W, V of the last update: ekf_peek_workspace) too.  (tools/determinism_probe.py
    is the long version: 5440 frames without a deviation, profiles/r5_determinism_probe.txt.)"""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    n_feat, frames = 1000, 6
    px0, z = synthetic.measurement_stream(cfg, n_feat, frames, sigma_px=0.5)

    def run():
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat + 16)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        rng = np.random.default_rng(7)
        sid = np.arange(n_feat)
        for k in range(frames):
            f.predict()
            sel = np.nonzero(sid >= 0)[0].astype(np.int32)
            f.update(z[k][sid[sel]].reshape(-1), sel)
            if k == 2:
                drop = sorted(rng.choice(n_feat, size=n_feat // 100, replace=False).tolist())
                f.removeFeatures(drop)
                sid = np.delete(sid, drop)
                for _ in drop:
                    assert f.addFeature((float(rng.uniform(20, 300)), float(rng.uniform(20, 220)))) == 1
                sid = np.concatenate([sid, -np.ones(len(drop), np.int64)])
        f.synchronize()
        n, mp = f.stateDim(), (2 * int(np.sum(sid >= 0)) + 127) // 128 * 128
        out = (f.getFullState(), f.getFullSigma(), f.peekWorkspace(0, 0, 0, n, mp), f.peekWorkspace(1, 0, 0, n, mp))
        f.close()
        return out

    a, b = run(), run()
    for x, y, name in zip(a, b, ("mu", "Sigma", "W", "V")):
        assert np.array_equal(x, y), f"{name}: {int(np.sum(x != y))} entries differ between two runs of the same calls"
    assert np.any(a[2] != 0) and np.any(a[3] != 0)


def test_profile_reports_time_and_work_of_the_downdate():
    """EKF_OPT_PROFILE = 1 times the downdate launches with HIP events; ekf_profile_work reports their algorithmic
    flop: n^2 x the measured columns (symmetric half) plus, for the launch that carries its chunk's W update,
    2 (n + 1) (m - c1) x its columns -- bench.py's roofline is the ratio of the two."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    n_feat = 640
    px0, z = synthetic.measurement_stream(cfg, n_feat, 3, sigma_px=0.5)
    f = pkg.VSlamFilter(cfg, capacity_features=n_feat)
    f.setDt(1.0 / 30.0)
    for (u, v) in px0:
        assert f.addFeature((u, v)) == 1
    idx = np.arange(n_feat, dtype=np.int32)
    f.set_option(2, 1)
    f.profile_reset()
    frames = 2
    for k in range(frames):
        f.predict()
        f.update(z[k].reshape(-1), idx)
    f.synchronize()
    prof, work = f.profile(), f.profile_work()
    ms, cnt = prof["downdate_syrk"]
    n, m = 14 + 6 * n_feat, 2 * n_feat
    assert cnt == 3 * frames and ms > 0                          # 10 block steps: three chunks, one downdate launch each
    lo = frames * float(n) * n * m                               # the symmetric downdate alone
    hi = lo + frames * 2.0 * (n + 1) * m * m                     # no W update is larger than 2 (n + 1) m^2
    assert lo <= work["downdate_syrk"] <= hi
    assert set(work) == {"downdate_syrk"}
    f.profile_reset()
    assert f.profile_work() == {} and "downdate_syrk" not in f.profile()


def test_largest_config_n4000_properties():
    """BASELINE configs[4] size on one GPU (N = M = 4000, n = 24014, 63 block steps, 2 x 2.3 GB of Sigma):
    one predict + update + a resize; the same size-independent properties as the N = 1000 test."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    N = 4000
    px0, z = synthetic.measurement_stream(cfg, N, 2, sigma_px=0.5)
    f = pkg.VSlamFilter(cfg, capacity_features=N)
    f.setDt(1.0 / 30.0)
    for (u, v) in px0:
        assert f.addFeature((u, v)) == 1
    with pytest.raises(Exception):
        f.addFeature((100.0, 100.0))                        # capacity_features is a hard bound
    assert f.numOfFeatures() == N and f.stateDim() == 14 + 6 * N
    f.predict()
    h, vis, rem, S2 = f.predictions()
    assert vis.sum() >= 0.98 * N
    d_pred = np.diag(f.getSigmaBlock(14, 14, 600, 600)).copy()
    f.update(z[0].reshape(-1), np.arange(N, dtype=np.int32))
    f.synchronize()                                         # raises if a Cholesky pivot was not positive
    mu = f.getFullState()
    assert np.all(np.isfinite(mu)) and abs(np.linalg.norm(mu[3:7]) - 1.0) < 1e-6
    S = f.getSigmaBlock(0, 0, 620, 620)
    assert np.abs(S - S.T).max() <= 1e-6 * np.abs(S).max()
    d = np.diag(S)
    assert np.all(d > 0) and np.all(d[14:614] <= d_pred * (1 + 1e-5))
    far = f.getSigmaBlock(24014 - 300, 0, 300, 300)          # a block far from the diagonal against its mirror
    assert bound("far, f.getSigmaBlock(0, 24014 - 300, 300, 300).T", relf(far, f.getSigmaBlock(0, 24014 - 300, 300, 300).T), 1e-6)
    f.removeFeatures([5, 1999, 3999])                        # one compaction pass over 2.3 GB
    assert f.numOfFeatures() == N - 3 and f.stateDim() == 14 + 6 * (N - 3)
    f.predict()
    h, vis, rem, S2 = f.predictions()
    assert np.all(np.isfinite(h)) and vis.sum() >= 0.98 * (N - 3)


def test_n4000_matches_fp64_oracle_sketch():
    """BASELINE configs[4] size against the ORACLE (VERDICT r3 next #1b): N = M = 4000, n = 24 014, 63 block steps, the
    long-chain chunk plan, two frames (predict + update; the second one sees parallax, so the inverse depths move) of the
    bench stream, fp32 with every option at its default (the map built
    by the filter's own 4000 fp32 adds) -- against the fp64 structured oracle's result, which
    tools/n4000_oracle_parity.py --write-golden stored as tests/golden/n4000_oracle_sketch.npz (the oracle needs ~5 min and
    19 GB of host memory: too slow for this suite; the FULL entry-by-entry comparison of the same run is
    profiles/r4_n4000_oracle_parity.txt, `--hip` of that script).  Compared: mu, diag(Sigma), eight full rows of Sigma
    (camera, first / middle / last feature) and Sigma R for four seeded Gaussian vectors, whose error norm estimates the
    Frobenius error of the whole matrix (E |D r|^2 = |D|_F^2)."""
    from __graft_entry__ import load_package
    pkg = load_package()
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import n4000_oracle_parity as npar
    g = np.load(npar.GOLDEN)
    N = npar.N
    _, px0, z = npar.stream()
    f = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=N)
    f.setDt(1.0 / 30.0)
    for (u, v) in px0:
        assert f.addFeature((u, v)) == 1
    for k in range(npar.FRAMES):
        f.predict()
        f.update(z[k].reshape(-1), np.arange(N, dtype=np.int32))
    f.synchronize()                                         # raises if a Cholesky pivot was not positive
    mu = f.getFullState()
    S = f.getFullSigma()
    pad, asym, big = f.checkInvariants()
    f.close()
    assert pad == 0.0 and asym == 0.0
    t = TOL[np.float32]
    # ceilings of two fp32 frames on a map of 4000 fp32 adds (N = 1000 measured 1.8e-6 / 3.2e-5 after its second frame) -- and,
    # round 5, the YARDSTICK of SURVEY 8c beside every figure: the fp32 structured ORACLE's own distance from the fp64
    # oracle on the same run (o32_* in the fixture; tools/n4000_oracle_parity.py --write-golden): the HIP filter must
    # stay within 1.5 x that distance plus one single-step tolerance, as at N = 1000
    def yard(key, tol):
        return 1.5 * float(g[key]) + tol
    e_mu = relf(mu, g["mu"])
    assert bound("mu vs fp64 oracle", e_mu, 2 * t["mu"]) and e_mu <= yard("o32_rel_mu", t["mu"]), (e_mu, float(g["o32_rel_mu"]))
    e_d = relf(np.diag(S), g["diag"])
    assert bound("diag(Sigma) vs fp64 oracle", e_d, 5 * t["S"]) and e_d <= yard("o32_rel_diag", t["S"]), (e_d, float(g["o32_rel_diag"]))
    rows = [int(r) for r in g["rows_idx"]]
    e_r = relf(S[rows], g["rows"])
    assert bound("eight rows of Sigma vs fp64 oracle", e_r, 5 * t["S"]) and e_r <= yard("o32_rel_rows", t["S"]), (e_r, float(g["o32_rel_rows"]))
    for k, r in enumerate(rows[4:]):                        # feature rows one by one (a camera row would hide them)
        e_k = relf(S[r], g["rows"][k + 4])
        assert bound(f"Sigma row {k + 4} of the sketch vs fp64 oracle", e_k, 25 * t["S"])   # one row: first run 1.3e-4
        # (single rows scatter: the fp32 oracle is between 2.1e-5 and 2.4e-4 from the fp64 one on these four, the HIP filter
        # between 3e-5 and 1.3e-4, not on the same rows -- the yardstick for ONE row is the fp32 oracle's worst feature row)
        assert e_k <= 1.5 * float(np.max(g["o32_rel_row_each"][4:])) + t["S"], (k, e_k, g["o32_rel_row_each"][4:].tolist())
    proj = npar.blocked_matmul(S, npar.sketch_matrix(S.shape[0]))
    e_p = relf(proj, g["proj"])
    assert bound("Sigma R (4 Gaussian vectors) vs fp64 oracle", e_p, 10 * t["S"]) and e_p <= yard("o32_rel_proj", t["S"]), (e_p, float(g["o32_rel_proj"]))
    # the sketch's estimate of |Sigma_hip - Sigma_oracle|_F / |Sigma_oracle|_F
    est = float(np.linalg.norm(proj - g["proj"]) / np.sqrt(proj.shape[1]) / float(g["fro"]))
    assert bound("estimated rel. Frobenius error of Sigma vs fp64 oracle", est, 5 * t["S"])
    assert est <= yard("o32_est_fro", t["S"]), (est, float(g["o32_est_fro"]))


def test_split_bf16_downdate_is_fp32_accurate():
    """EKF_OPT_SPLIT_BF16 (default 1 since round 5): the downdate on the bf16 matrix pipe with 3 x bf16 operands
    (k_syrk_bf16x6) against the exact-fp32 arithmetic (option 0: k_gemm_mfma<DOWNDATE> on v_mfma_f32_32x32x2_f32).  BOTH
    are measured against the fp64 oracle on the same inputs: each within the fp32 tolerances, the bf16x6 path within a
    small factor of the fp32 instruction's own error -- and the launch counters prove that each filter ran the kernel its
    label names (round 5's default flip had turned this test into a self-comparison: VERDICT r5 weak #1)."""
    n_feat = 530                                             # 25 tile rows: the split kernel is used from 23 up
    ref, g0 = make_pair(n_feat, np.float32, capacity=n_feat)
    ref64 = o.build_scenario(o.StructuredFilter, oracle_cfg(), n_feat, np.float64)
    _, g1 = make_pair(n_feat, np.float32, capacity=n_feat)
    g0.set_option(4, 0)                                      # exact fp32
    g1.set_option(4, 1)                                      # bf16 x 6 (the default, set explicitly)
    ref64.predict()
    vis = ref64.visible_indices()
    z = o.synthetic_measurements(ref64, vis, seed=1235, sigma=0.5)
    ref64.update(z, vis)
    errs = []
    for g in (g0, g1):
        g.setFullState(ref.mu)                               # identical fp32 inputs on both
        g.setSigmaBlock(ref.Sigma)
        g.profile_reset()
        g.predict()
        g.update(z.astype(np.float32), vis)
        g.synchronize()
        mu, S = gpu_state(g)
        errs.append((relf(mu, ref64.mu), relf(S, ref64.Sigma), np.abs(S - S.T).max() / np.abs(S).max(), mu, S))
    c0, c1 = g0.launch_counts(), g1.launch_counts()
    f32_kinds = ("downdate_f32", "downdate_f32_fused_wu", "downdate_f32_half_tail")
    assert c0["downdate_bf16x6"] == 0 and sum(c0[k] for k in f32_kinds) >= 1, c0
    assert c1["downdate_bf16x6"] >= 1 and sum(c1[k] for k in f32_kinds) == 0, c1
    (mu0, s0, a0, m0, S0), (mu1, s1, a1, m1, S1) = errs
    assert not np.array_equal(S0, S1)                        # two arithmetics, two results
    t = TOL[np.float32]
    assert bound("exact fp32 path mu vs fp64 oracle", mu0, t["mu"]) and bound("exact fp32 path Sigma vs fp64 oracle", s0, t["S"])
    assert bound("bf16x6 path mu vs fp64 oracle", mu1, t["mu"]) and bound("bf16x6 path Sigma vs fp64 oracle", s1, t["S"])
    assert a0 == 0.0 and a1 == 0.0                           # both exactly symmetric
    assert s1 < 3 * s0 + 1e-6 and mu1 < 3 * mu0 + 1e-6, errs[0][:3] + errs[1][:3]


def test_n1000_exact_fp32_downdate_matches_fp64_oracle():
    """The exact-fp32 large-map path (EKF_OPT_SPLIT_BF16 = 0: k_gemm_mfma<DOWNDATE, 128 x 128>, its fused innovation-row
    launch and the half-tile tail -- `bench.py --exact-fp32`, and what a rank without rows falls back to) at the HEADLINE
    size against the fp64 structured oracle: N = M = 1000, two frames of the bench stream, with the fp32 structured
    oracle's own distance from the fp64 one as the yardstick, as the default arithmetic has it in
    test_n1000_default_pipeline_matches_fp64_oracle.  (vR.cpp:1279)"""
    from __graft_entry__ import load_package
    pkg = load_package()
    import helpers
    px0, z, states = helpers.n1000_oracle(2)
    yard = helpers.n1000_yardstick(2)
    N = 1000
    f = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=N)
    f.setDt(1.0 / 30.0)
    f.set_option(4, 0)
    for (u, v) in px0:
        assert f.addFeature((u, v)) == 1
    idx = np.arange(N, dtype=np.int32)
    for k in range(2):
        f.predict()
        f.update(z[k].reshape(-1).astype(np.float32), idx)
        f.synchronize()
        mu, S = gpu_state(f)
        mu64, S64 = states[k + 1]
        e_mu, e_S = relf(mu, mu64), relf(S, S64)
        y_mu, y_S = yard[k]
        print(f"N=1000 exact fp32, frame {k}: HIP-o64 mu {e_mu:.2e} Sigma {e_S:.2e} | o32-o64 mu {y_mu:.2e} Sigma {y_S:.2e}", flush=True)
        c = k + 1
        assert bound(f"frame {k}: mu vs fp64 oracle", e_mu, c * TOL[np.float32]["mu"])
        assert bound(f"frame {k}: Sigma vs fp64 oracle", e_S, c * 2.5 * TOL[np.float32]["S"])
        assert e_S <= 1.5 * y_S + TOL[np.float32]["S"], (k, e_S, y_S)
        assert e_mu <= 1.5 * y_mu + TOL[np.float32]["mu"], (k, e_mu, y_mu)
        assert np.array_equal(S, S.T)
    c = f.launch_counts()
    assert c["downdate_bf16x6"] == 0 and c["downdate_f32_fused_wu"] >= 1 and c["downdate_f32_half_tail"] >= 1, c
    pad, asym, big = f.checkInvariants()
    assert pad == 0.0 and asym == 0.0
    f.close()


# ---------------------------------------------------------------------------------------------
# Oracle parity at the HEADLINE size through the production launch structure (VERDICT r2 next #1a, r3 next #1a):
# N = M = 1000, n = 6014, fp32, default options -- 16 block steps in three chunks, the fused first launch, half
# tiles, the CU-masked second stream -- against the fp64 structured oracle on the same inputs, TEN frames, with the
# fp32 structured oracle run beside it from the same start as the yardstick (tolerances are calibrated
# against the fp32-oracle-vs-fp64-oracle gap).
# ---------------------------------------------------------------------------------------------
N1000_FRAMES = 10


def test_n1000_default_pipeline_matches_fp64_oracle():
    from threadpoolctl import threadpool_limits
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    import helpers
    import oracle_worker
    N, frames = 1000, N1000_FRAMES
    # z rounded to fp32 once: the fp64 oracle, the fp32 oracle and the HIP filter read the SAME numbers
    px0, z = synthetic.measurement_stream(pkg.kinect_config(), N, frames, sigma_px=0.5, dtype=np.float32)
    refs = {}
    for T in (np.float64, np.float32):
        r = o.StructuredFilter(o.Config.kinect(), T)
        r.dT = 1.0 / 30.0
        assert r.add_features(px0) == N
        refs[T] = r
    ref64, ref32 = refs[np.float64], refs[np.float32]
    f = pkg.VSlamFilter(pkg.kinect_config(), capacity_features=N)          # fp32, every option at its default
    f.setDt(1.0 / 30.0)
    for (u, v) in px0:
        assert f.addFeature((u, v)) == 1
    f.synchronize()
    # the HIP filter built its map with its OWN fp32 add-feature path: that map against the oracle's
    mu, S = gpu_state(f)
    assert bound("map after 1000 adds: mu", relf(mu, ref64.mu), TOL[np.float32]["mu"])
    assert bound("map after 1000 adds: Sigma", relf(S, ref64.Sigma), TOL[np.float32]["S"])
    states = [(ref64.mu.copy(), ref64.Sigma.copy())]
    limiter = threadpool_limits(limits=16)
    rows = []
    for k in range(frames):
        for r in (ref64, ref32):
            oracle_worker.predict_no_St(r)                # St is recomputed by the update (vR.cpp:1268)
        f.predict()
        # every VISIBLE feature is measured (from the third frame on a few features leave the margin of the image)
        vis = ref64.visible_indices()
        assert ref32.visible_indices() == vis and len(vis) >= N - 20
        h, gvis, grem, _ = f.predictions()
        assert list(np.nonzero(gvis)[0]) == vis, k
        if k < 2:
            assert len(vis) == N                         # (the sharded N = 1000 tests share these two frames: all measured)
        zk = z[k][vis].reshape(-1)
        for r in (ref64, ref32):
            r.update(zk.astype(r.T), vis)
        f.update(zk, np.asarray(vis, np.int32))
        f.synchronize()
        mu, S = gpu_state(f)
        if k < 2:                                        # shared with the sharded N = 1000 tests (helpers.n1000_oracle)
            states.append((ref64.mu.copy(), ref64.Sigma.copy()))
            if k == 1:
                helpers._N1000_ORACLE[2] = (px0, z[:2].astype(np.float64), states)
        e_mu, e_S = relf(mu, ref64.mu), relf(S, ref64.Sigma)
        e_Sf = relf(S[14:, 14:], ref64.Sigma[14:, 14:])
        y_mu, y_S = relf(ref32.mu, ref64.mu), relf(ref32.Sigma, ref64.Sigma)      # the fp32 ORACLE against the truth
        g_mu, g_S = relf(mu, ref32.mu), relf(S, ref32.Sigma)
        rows.append((k, e_mu, e_S, y_mu, y_S, g_mu, g_S))
        print(f"N=1000 frame {k}: HIP-o64 mu {e_mu:.2e} Sigma {e_S:.2e} | o32-o64 mu {y_mu:.2e} Sigma {y_S:.2e} | "
              f"HIP-o32 mu {g_mu:.2e} Sigma {g_S:.2e}", flush=True)
        # ceilings: one fp32 predict + update on top of a map built by 1000 fp32 adds; every later frame carries the
        # rounding of the frames before it (measured growth: profiles/r4_parity_measured.jsonl; parity_bounds.json
        # holds each site to 10 x what the MI355X measured)
        c = min(k + 1, 4)
        assert bound(f"frame {k}: mu vs fp64 oracle", e_mu, c * TOL[np.float32]["mu"])
        assert bound(f"frame {k}: Sigma vs fp64 oracle", e_S, c * 2.5 * TOL[np.float32]["S"])
        assert np.array_equal(S, S.T)                    # exactly symmetric
        # the feature block alone (the camera block is 1e3 larger in norm and would hide an error there)
        assert bound(f"frame {k}: Sigma[features] vs fp64 oracle", e_Sf, c * 2.5 * TOL[np.float32]["S"])
        # the yardstick: the HIP fp32 path is no farther from the fp64 truth than the reference's fp32 formulation
        # (1.5 x, + the single-frame tolerance), and its distance from the fp32 oracle is explained by that oracle's own
        assert e_S <= 1.5 * y_S + TOL[np.float32]["S"], rows[-1]
        assert e_mu <= 1.5 * y_mu + TOL[np.float32]["mu"], rows[-1]
        assert g_S <= 1.5 * y_S + c * 2.5 * TOL[np.float32]["S"], rows[-1]
        assert g_mu <= 1.5 * y_mu + c * TOL[np.float32]["mu"], rows[-1]
    limiter.restore_original_limits()
    pad, asym, big = f.checkInvariants()
    assert pad == 0.0 and asym == 0.0


@pytest.mark.parametrize("n_feat", [30, 62, 63, 200])
def test_fused_launches_match_launch_per_kernel(n_feat):
    """EKF_OPT_FUSED_LAUNCHES (default on): (a) camera step + strip congruence + per-feature h / H of ekf_predict as ONE
    launch is bit-identical to the three (every workgroup repeats the same one-lane camera step); (b) with the
    innovation inside one 128-column block (n_feat = 30: 2 M + 3 = 63) the solve + state update go out as one launch
    without the panel step -- the same sums in another order: fp32 rounding, and the gain / the strip the general path
    leaves are there too.  n_feat = 62 / 63 sit at the edge (2 M <= 128 measured rows: whether a frame takes the one-block
    path depends on how many features are visible); n_feat = 200 (four blocks) only has (a), so that run stays bit-identical."""
    ref, g1 = make_pair(n_feat, np.float32)
    _, g0 = make_pair(n_feat, np.float32)
    g0.set_option(6, 0)                                          # one launch per kernel
    seen_oneblock = False
    # n_feat = 200 (round 5): "frame 1: Sigma vs oracle" sat at 3.5e-5 of its 4e-5 ceiling for two rounds
    # -- against the fp32 ORACLE.  An fp64 oracle on the same fp32-valued start and the same measurements says whose error
    # that is: the HIP filter is held to 1.5 x the fp32 oracle's own distance from it plus one single-step tolerance
    ref64 = None
    if n_feat == 200:
        ref64 = o.build_scenario(o.StructuredFilter, oracle_cfg(), n_feat, np.float64)
        ref64.mu = ref.mu.astype(np.float64).copy()
        ref64.Sigma = ref.Sigma.astype(np.float64).copy()
    for k in range(3):
        ref.predict()
        if ref64 is not None:
            ref64.predict()
        g1.predict()
        g0.predict()
        mu1, S1 = gpu_state(g1)
        mu0, S0 = gpu_state(g0)
        p1, p0 = g1.predictions(jacobians=True), g0.predictions(jacobians=True)
        Ft1, Q1 = g1.motionJacobian()
        Ft0, Q0 = g0.motionJacobian()
        if not seen_oneblock:                                    # same state in: same bits out
            assert np.array_equal(Ft1, Ft0) and np.array_equal(Q1, Q0)
            assert np.array_equal(mu1, mu0) and np.array_equal(S1, S0)
            for a, b in zip(p1, p0):
                assert np.array_equal(np.asarray(a), np.asarray(b))
        vis = ref.visible_indices()
        z = o.synthetic_measurements(ref, vis, seed=500 + k)
        ref.update(z, vis)
        g1.update(z, vis)
        g0.update(z, vis)
        mu1, S1 = gpu_state(g1)
        mu0, S0 = gpu_state(g0)
        if 2 * len(vis) > 128:                                   # (the one-block path goes by the MEASURED rows)
            assert np.array_equal(mu1, mu0) and np.array_equal(S1, S0)
        else:
            seen_oneblock = True
            assert bound(f"frame {k}: mu fused vs launch-per-kernel", relf(mu1, mu0), 2e-6 * (k + 1))
            assert bound(f"frame {k}: Sigma fused vs launch-per-kernel", relf(S1, S0), 5e-6 * (k + 1))
            assert bound(f"frame {k}: gain fused vs launch-per-kernel", relf(g1.getGain(), g0.getGain()), 1e-4 * (k + 1))
        assert bound(f"frame {k}: mu vs oracle", relf(mu1, ref.mu), TOL[np.float32]["mu"] * 5 * (k + 1))
        assert bound(f"frame {k}: Sigma vs oracle", relf(S1, ref.Sigma), TOL[np.float32]["S"] * (k + 1))
        if ref64 is not None:
            ref64.update(z.astype(np.float64), vis)
            e64, o32 = relf(S1, ref64.Sigma), relf(ref.Sigma, ref64.Sigma)
            assert bound(f"frame {k}: Sigma vs fp64 oracle", e64, TOL[np.float32]["S"] * (k + 1))
            assert e64 <= 1.5 * o32 + TOL[np.float32]["S"], (k, e64, o32)
            assert bound(f"frame {k}: mu vs fp64 oracle", relf(mu1, ref64.mu), TOL[np.float32]["mu"] * 5 * (k + 1))
            print(f"[fused_launches 200] frame {k}: |HIP - o64| {e64:.2e}  |o32 - o64| {o32:.2e}  |HIP - o32| {relf(S1, ref.Sigma):.2e}")
        assert np.array_equal(S1, S1.T)
    g1.synchronize()
    g0.synchronize()


def test_two_group_solve_agrees_with_the_single_group_solve(monkeypatch):
    """Latency-bound solve launches run every tile on two groups of four waves, each taking every second K step
    (k_gemm_mfma<.., S2>): the same products summed in two partial sums, i.e. fp32 rounding against the one-group kernel
    (EKF_SOLVE_S2=0), and the selection rule looks only at the chunk width and the size of the whole state, so it cannot
    differ between the plain and the sharded path (their bit-identity is asserted in tests/test_sharded.py)."""
    from __graft_entry__ import load_package
    pkg = load_package()
    from ekf_monoslam_amd import synthetic
    cfg = pkg.kinect_config()
    n_feat = 640
    px0, z = synthetic.measurement_stream(cfg, n_feat, 3, sigma_px=0.5)
    idx = np.arange(n_feat, dtype=np.int32)
    outs = []
    for mode in ("1", "0"):
        monkeypatch.setenv("EKF_SOLVE_S2", mode)             # read when the filter is created
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat)
        f.setDt(1.0 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        for k in range(2):
            f.predict()
            f.update(z[k].reshape(-1), idx)
        f.synchronize()
        outs.append((f.getFullState(), f.getFullSigma()))
        f.close()
    monkeypatch.delenv("EKF_SOLVE_S2", raising=False)
    assert not np.array_equal(outs[0][1], outs[1][1])        # the two-group path did run
    assert bound("mu two-group vs one-group solve", relf(outs[0][0], outs[1][0]), 5e-6)
    assert bound("Sigma two-group vs one-group solve", relf(outs[0][1], outs[1][1]), 2e-5)
    assert np.array_equal(outs[0][1], outs[0][1].T)


def test_host_inputs_through_the_pinned_ring_without_synchronisation():
    """ekf_update stages host z / indices through a ring of four pinned slots and returns at once; ten frames are queued
    without any read-back or synchronisation in between (the ring wraps twice, the caller's buffer is overwritten right
    after every call), then the state is compared with the oracle's."""
    ref, g = make_pair(24, np.float32)
    zbuf = np.zeros(2 * 24, np.float32)
    for k in range(10):
        ref.predict()
        g.predict()
        vis = ref.visible_indices()
        z = o.synthetic_measurements(ref, vis, seed=900 + k)
        ref.update(z, vis)
        zbuf[:z.size] = np.asarray(z, np.float32).reshape(-1)
        g.update(zbuf[:z.size], vis)
        zbuf[:] = np.nan                                         # the call has copied its inputs: this must not matter
    g.synchronize()
    mu, S = gpu_state(g)
    assert bound("mu after 10 queued frames", relf(mu, ref.mu), TOL[np.float32]["mu"] * 20)
    assert bound("Sigma after 10 queued frames", relf(S, ref.Sigma), TOL[np.float32]["S"] * 10)
    g.predict()
    h, vis_g, rem, S2 = g.predictions()                           # the read-back buffer after the queue has drained
    assert np.all(np.isfinite(h)) and np.all(np.isfinite(S2))
