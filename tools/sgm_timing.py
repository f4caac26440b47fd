"""Timing of the semi-global sweep (k_sweep_volume, one k_sgm_path per direction and k_sgm_winner behind
ekf_dense_sweep_sgm) on the step scene of tests/dense_scene.py rendered at 640 x 480 (D = 128, radius 2, 4 sources, 8 paths)
and 320 x 240 (D = 64, radius 2, 2 sources, 8 paths).  Per case, the mean HIP-event times over --reps calls
(ekf_dense_profile): the volume sweep beside the plain k_plane_sweep of the same arguments, every direction's launch with
the bytes it moves (the first direction reads C and writes S, each later one also reads S: 4 bytes an element each) and the
share of the HBM peak that implies, and the winner.  No gate: the parent has no such path.
Usage: python tools/sgm_timing.py [--reps 20] [--out profiles/sgm_timing_mi355x.json]"""
import argparse, json, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "oracle"), os.path.join(R, "tests"), os.path.join(R, "tools")]
from __graft_entry__ import load_package
import dense_scene as ds
from dense_timing import rig

pkg = load_package()
HBM_PEAK_GBS = 8000.0                                   # MI355X: 8 TB/s


def run(name, w, h, D, radius, n_src, paths, reps):
    K = np.array([ds.K[0] * w / ds.W, ds.K[1] * w / ds.W, (w - 1) / 2.0, (h - 1) / 2.0])
    views = ds.step_scene(rig(n_src), Kc=K, w=w, h=h)
    d = pkg.DenseStereo(w, h, n_src + 1)
    for s, v in views.items():
        d.set_view(s, *v)
    src = sorted(views)[1:]
    d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, 40)                  # warm-ups: both code paths, the volumes allocated
    d.sweep_sgm(0, src, ds.W_MIN, ds.W_MAX, D, radius, 40, paths=paths)
    d.profile(True)
    for _ in range(reps):
        d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, 40)
        d.sweep_sgm(0, src, ds.W_MIN, ds.W_MAX, D, radius, 40, paths=paths)
    plain, prof = d.get_profile(), d.get_sgm_profile()
    d.profile(False)
    d.close()
    assert plain["k_plane_sweep"][1] == reps and prof["k_sweep_volume"][1] == reps and prof["k_sgm_winner"][1] == reps, (plain, prof)
    elems = w * h * D
    row = {"case": name, "width": w, "height": h, "planes": D, "radius": radius, "sources": n_src, "paths": paths, "reps": reps,
           "k_plane_sweep_ms": plain["k_plane_sweep"][0] / reps, "k_sweep_volume_ms": prof["k_sweep_volume"][0] / reps,
           "k_sgm_winner_ms": prof["k_sgm_winner"][0] / reps, "directions": []}
    for i in range(paths):
        ms, n = prof["k_sgm_path[%d]" % i]
        assert n == reps, prof
        moved = elems * 4 * (2 if i == 0 else 3)
        row["directions"].append({"direction": i, "ms": ms / reps, "bytes": moved,
                                  "hbm_peak_share": moved / (ms / reps * 1e-3) / (HBM_PEAK_GBS * 1e9)})
    row["k_sgm_path_ms_total"] = sum(x["ms"] for x in row["directions"])
    row["sweep_sgm_ms_total"] = row["k_sweep_volume_ms"] + row["k_sgm_path_ms_total"] + row["k_sgm_winner_ms"]
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run("640x480 D=128 r=2 V=4 paths=8", 640, 480, 128, 2, 4, 8, a.reps),
            run("320x240 D=64 r=2 V=2 paths=8", 320, 240, 64, 2, 2, 8, a.reps)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/sgm_timing.py", "hbm_peak_gb_s": HBM_PEAK_GBS, "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
