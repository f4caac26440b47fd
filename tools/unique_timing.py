"""Timing of the runner-up cost and the uniqueness test (the four twins of the pixel-wise sweeps,
k_sgm_winner_unique and k_depth_filter_unique behind ekf_dense_keep_runner_up and ekf_dense_filter_unique) on the step scene of
tests/dense_scene.py rendered at 640 x 480 (D = 128, radius 2, 4 sources, n_best 2) and 320 x 240 (D = 64, radius 2, 2 sources,
n_best 1), the shapes of tools/best_timing.py.  Per case, the mean HIP-event times over --reps calls (ekf_dense_profile) of
each new kernel, with the kernel it stands in for beside it: the same arguments, the same session, the switch off and on in
turn.  The descriptors are fresh, so no k_census runs inside the timed calls.  No gate: the parent has no such path.
Usage: python tools/unique_timing.py [--reps 50] [--out profiles/unique_timing_mi355x.json]"""
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

    def calls(keep):
        d.keep_runner_up(keep)
        for cost in ("ad", "census"):
            for best in (None, n_best):
                d.sweep(*args, cost=cost, best=best)
        d.sweep_sgm(*args)
        d.filter(0, src, 0.01, 1, uniqueness=5 if keep else 0)      # of the aggregated map, which has its runner-up

    for s in src:                                                   # the filter reads the sources' swept depths
        d.sweep(s, [0] + [o for o in src if o != s], ds.W_MIN, ds.W_MAX, D, radius, 40)
    calls(False), calls(True)                                       # warm-ups: every code path, every buffer allocated
    d.profile(True)
    for _ in range(reps):
        calls(False), calls(True)
    plain, sgm, census, best, uniq = (d.get_profile(), d.get_sgm_profile(), d.get_census_profile(), d.get_best_profile(),
                                      d.get_unique_profile())
    d.profile(False)
    d.close()
    per = lambda prof, k: prof[k][0] / max(prof[k][1], 1)
    assert uniq["k_sgm_winner_unique"][1] == reps and sgm["k_sgm_winner"][1] == reps, (uniq, sgm)
    assert uniq["k_depth_filter_unique"][1] == reps and plain["k_depth_filter_points"][1] == reps, (uniq, plain)
    assert [uniq[k][1] for k in list(uniq)[1:4]] == [reps] * 3 and census["k_census"][1] == 0, (uniq, census)
    row = {"case": name, "width": w, "height": h, "planes": D, "radius": radius, "sources": n_src, "n_best": n_best, "reps": reps,
           "k_plane_sweep_ms": per(plain, "k_plane_sweep"), "k_plane_sweep_census_ms": per(census, "k_plane_sweep_census"),
           "k_plane_sweep_best_ms": per(best, "k_plane_sweep_best"), "k_plane_sweep_best_census_ms": per(best, "k_plane_sweep_best_census"),
           "k_sgm_winner_ms": per(sgm, "k_sgm_winner"), "k_depth_filter_points_ms": per(plain, "k_depth_filter_points")}
    row.update({k + "_ms": per(uniq, k) for k in uniq})
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run("640x480 D=128 r=2 V=4 best=2", 640, 480, 128, 2, 4, 2, a.reps),
            run("320x240 D=64 r=2 V=2 best=1", 320, 240, 64, 2, 2, 1, a.reps)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/unique_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
