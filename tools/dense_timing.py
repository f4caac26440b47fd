"""Timing of the dense plane sweep (k_plane_sweep behind ekf_dense_sweep, k_depth_filter_points behind
ekf_dense_filter) on the step scene of tests/dense_scene.py rendered at 640 x 480 (D = 128, radius 2, 4 sources) and
320 x 240 (D = 64, radius 2, 2 sources).  Per case: the mean HIP-event time of the two kernels over --reps calls
(ekf_dense_profile), the warps per second that makes (W H D V per sweep), and the share of the filter in sweep + filter.
Beside it, for the 61 x 47 test shape only, the device sweep and the wall time of the numpy oracle on this host.  No gate:
the parent has no such path.
Usage: python tools/dense_timing.py [--reps 50] [--out profiles/dense_timing_mi355x.json]"""
import argparse, json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "oracle"), os.path.join(R, "tests")]
from __graft_entry__ import load_package
import dense_oracle as do
import dense_scene as ds

pkg = load_package()


def rig(n_src):
    """The reference at the origin and n_src cameras on a sideways line, alternating sides, slightly rotated."""
    poses = {0: ds.REF}
    for i in range(n_src):
        side = 1.0 if i % 2 == 0 else -1.0
        poses[i + 1] = ds._pose([side * ds.BASELINE * (1 + i // 2) / 2.0, 0.01 * i, 0.0], [0.0, -0.01 * side, 0.002 * i])
    return poses


def run(name, w, h, D, radius, n_src, reps, oracle=False):
    K = np.array([ds.K[0] * w / ds.W, ds.K[1] * w / ds.W, (w - 1) / 2.0, (h - 1) / 2.0])
    views = ds.step_scene(rig(n_src), Kc=K, w=w, h=h)
    d = pkg.DenseStereo(w, h, n_src + 1)
    for s, v in views.items():
        d.set_view(s, *v)
    slots = sorted(views)
    sweep = lambda r: d.sweep(r, [s for s in slots if s != r], ds.W_MIN, ds.W_MAX, D, radius, 40)
    for r in slots:                                     # every source swept once: the filter needs their maps (and a warm-up)
        sweep(r)
    d.profile(True)
    for _ in range(reps):
        sweep(0)
        d.filter(0, slots[1:], 0.02, 1)
    prof = d.get_profile()
    d.profile(False)
    assert prof["k_plane_sweep"][1] == reps and prof["k_depth_filter_points"][1] == reps, prof
    sweep_ms, filter_ms = prof["k_plane_sweep"][0] / reps, prof["k_depth_filter_points"][0] / reps
    row = {"case": name, "width": w, "height": h, "planes": D, "radius": radius, "sources": n_src, "reps": reps,
           "k_plane_sweep_ms": sweep_ms, "k_depth_filter_points_ms": filter_ms,
           "warps_per_s": w * h * D * n_src / (sweep_ms * 1e-3), "filter_share": filter_ms / (sweep_ms + filter_ms)}
    if oracle:
        got = d.depth(0)
        t0 = time.perf_counter()
        want = do.sweep(views[0][0], views[0][1], views[0][2], [views[s] for s in slots[1:]], ds.W_MIN, ds.W_MAX, D, radius, 40)
        row["numpy_oracle_wall_ms"] = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(got["depth"].view(np.uint32), want["depth"].view(np.uint32)), "device depth differs from the oracle"
    d.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run("640x480 D=128 r=2 V=4", 640, 480, 128, 2, 4, a.reps),
            run("320x240 D=64 r=2 V=2", 320, 240, 64, 2, 2, a.reps),
            run("61x47 D=12 r=2 V=2 (test shape, with the oracle)", ds.W, ds.H, ds.PLANES, 2, 2, a.reps, oracle=True)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/dense_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
