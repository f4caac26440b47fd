"""Timing of the best-K source selection (k_plane_sweep_best, k_plane_sweep_best_census, k_sweep_volume_best and
k_sweep_volume_best_census behind ekf_dense_sweep_best) on the step scene of tests/dense_scene.py rendered at 640 x 480
(D = 128, radius 2, 4 sources, n_best 2 and 4) and 320 x 240 (D = 64, radius 2, 2 sources, n_best 1), the shapes of
tools/census_timing.py.  Per case, the mean HIP-event times over --reps calls (ekf_dense_profile) of the four new kernels,
with k_plane_sweep, k_sweep_volume and their census twins of the same arguments beside them in the same session.  The
descriptors are fresh, so no k_census runs inside the timed calls.  No gate: the parent has no such path.
Usage: python tools/best_timing.py [--reps 50] [--out profiles/best_timing_mi355x.json]"""
import argparse, json, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "oracle"), os.path.join(R, "tests"), os.path.join(R, "tools")]
from __graft_entry__ import load_package
import dense_scene as ds
from dense_timing import rig

pkg = load_package()


def run(name, w, h, D, radius, n_src, n_best, reps):
    K = np.array([ds.K[0] * w / ds.W, ds.K[1] * w / ds.W, (w - 1) / 2.0, (h - 1) / 2.0])
    views = ds.step_scene(rig(n_src), Kc=K, w=w, h=h)
    d = pkg.DenseStereo(w, h, n_src + 1)
    for s, v in views.items():
        d.set_view(s, *v)
    src = sorted(views)[1:]
    args = (0, src, ds.W_MIN, ds.W_MAX, D, radius, 40)
    for cost in ("ad", "census"):                                  # warm-ups: every code path, every buffer allocated
        for best in (None, n_best):
            d.sweep(*args, cost=cost, best=best)
            d.sweep_sgm(*args, cost=cost, best=best)
    d.profile(True)
    for _ in range(reps):
        for cost in ("ad", "census"):
            for best in (None, n_best):
                d.sweep(*args, cost=cost, best=best)
                d.sweep_sgm(*args, cost=cost, best=best)
    plain, sgm, census, best = d.get_profile(), d.get_sgm_profile(), d.get_census_profile(), d.get_best_profile()
    d.profile(False)
    d.close()
    assert plain["k_plane_sweep"][1] == reps and sgm["k_sweep_volume"][1] == reps, (plain, sgm)
    assert [census[k][1] for k in census] == [0, reps, reps] and [best[k][1] for k in best] == [reps] * 4, (census, best)
    row = {"case": name, "width": w, "height": h, "planes": D, "radius": radius, "sources": n_src, "n_best": n_best, "reps": reps,
           "lds_layout": "all pairs of views resident, 28416 B",
           "k_plane_sweep_ms": plain["k_plane_sweep"][0] / reps, "k_sweep_volume_ms": sgm["k_sweep_volume"][0] / reps,
           "k_plane_sweep_census_ms": census["k_plane_sweep_census"][0] / reps,
           "k_sweep_volume_census_ms": census["k_sweep_volume_census"][0] / reps}
    row.update({k + "_ms": best[k][0] / reps for k in best})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run("640x480 D=128 r=2 V=4 best=2", 640, 480, 128, 2, 4, 2, a.reps),
            run("640x480 D=128 r=2 V=4 best=4", 640, 480, 128, 2, 4, 4, a.reps),
            run("320x240 D=64 r=2 V=2 best=1", 320, 240, 64, 2, 2, 1, a.reps)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/best_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
