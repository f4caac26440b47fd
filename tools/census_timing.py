"""Timing of the census matching cost (k_census, k_plane_sweep_census and k_sweep_volume_census behind
ekf_dense_sweep_census / ekf_dense_sweep_sgm_census) on the step scene of tests/dense_scene.py rendered at 640 x 480 (D = 128,
radius 2, 4 sources) and 320 x 240 (D = 64, radius 2, 2 sources), the cases of tools/sgm_timing.py.  Per case, the mean
HIP-event times over --reps calls (ekf_dense_profile) of the three census kernels, with k_plane_sweep and k_sweep_volume of the
same arguments beside them in the same session; every view's image is set again before each census sweep, so k_census runs
for all of them every time.  No gate: the parent has no such path.
Usage: python tools/census_timing.py [--reps 20] [--out profiles/census_timing_mi355x.json]"""
import argparse, json, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "oracle"), os.path.join(R, "tests"), os.path.join(R, "tools")]
from __graft_entry__ import load_package
import dense_scene as ds
from dense_timing import rig

pkg = load_package()


def run(name, w, h, D, radius, n_src, reps):
    K = np.array([ds.K[0] * w / ds.W, ds.K[1] * w / ds.W, (w - 1) / 2.0, (h - 1) / 2.0])
    views = ds.step_scene(rig(n_src), Kc=K, w=w, h=h)
    d = pkg.DenseStereo(w, h, n_src + 1)
    for s, v in views.items():
        d.set_view(s, *v)
    src = sorted(views)[1:]
    args = (0, src, ds.W_MIN, ds.W_MAX, D, radius, 40)
    for cost in ("ad", "census"):                                  # warm-ups: every code path, every buffer allocated
        d.sweep(*args, cost=cost)
        d.sweep_sgm(*args, cost=cost)
    d.profile(True)
    for _ in range(reps):
        d.sweep(*args)
        d.sweep_sgm(*args)
        for s, v in views.items():                                 # stale descriptors: k_census of every view
            d.set_view(s, *v)
        d.sweep(*args, cost="census")
        d.sweep_sgm(*args, cost="census")
    plain, sgm, census = d.get_profile(), d.get_sgm_profile(), d.get_census_profile()
    d.profile(False)
    d.close()
    assert plain["k_plane_sweep"][1] == reps and sgm["k_sweep_volume"][1] == reps, (plain, sgm)
    assert [census[k][1] for k in census] == [reps * (n_src + 1), reps, reps], census
    return {"case": name, "width": w, "height": h, "planes": D, "radius": radius, "sources": n_src, "reps": reps,
            "k_census_ms": census["k_census"][0] / census["k_census"][1],
            "k_plane_sweep_census_ms": census["k_plane_sweep_census"][0] / reps,
            "k_sweep_volume_census_ms": census["k_sweep_volume_census"][0] / reps,
            "k_plane_sweep_ms": plain["k_plane_sweep"][0] / reps, "k_sweep_volume_ms": sgm["k_sweep_volume"][0] / reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run("640x480 D=128 r=2 V=4", 640, 480, 128, 2, 4, a.reps), run("320x240 D=64 r=2 V=2", 320, 240, 64, 2, 2, a.reps)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/census_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
