"""Timing of the speckle filter (k_speckle_label, k_speckle_merge, k_speckle_count, k_speckle_apply behind
ekf_dense_filter_speckle and ekf_dense_speckle_host) at 640 x 480 and 320 x 240 on four inputs: (a) the filtered map of the
step scene of tests/dense_scene.py, swept as tools/unique_timing.py sweeps it (D = 128, radius 2, 4 sources; D = 64, 2
sources), at min_size 4, max_diff 1; (b) all one plane; (c) the serpentine of tests/speckle_scene.py; (d) the 0 / 5
checkerboard at max_diff 0, every pixel a segment.  Per input and kernel the median, least and largest HIP-event time over --reps
calls after --warmup calls (ekf_dense_profile, read call by call), with k_plane_sweep and k_depth_filter_points of the same shape
and session beside them.  No gate: the parent has no such path.
Usage: python tools/speckle_timing.py [--reps 50] [--warmup 5] [--out profiles/speckle_timing_mi355x.json]"""
import argparse, json, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "oracle"), os.path.join(R, "tests"), os.path.join(R, "tools")]
from __graft_entry__ import load_package
import dense_scene as ds
import speckle_scene as sc
from dense_timing import rig

pkg = load_package()


def stats(samples):
    a = np.sort(np.asarray(samples, np.float64))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1])}


def run(name, w, h, D, radius, n_src, reps, warmup):
    K = np.array([ds.K[0] * w / ds.W, ds.K[1] * w / ds.W, (w - 1) / 2.0, (h - 1) / 2.0])
    views = ds.step_scene(rig(n_src), Kc=K, w=w, h=h)
    d = pkg.DenseStereo(w, h, n_src + 1)
    for s, v in views.items():
        d.set_view(s, *v)
    src = sorted(views)[1:]
    for s in src:                                                   # the filter reads the sources' swept depths
        d.sweep(s, [0] + [o for o in src if o != s], ds.W_MIN, ds.W_MAX, D, radius, 40)
    sweep, filt = [], []
    for i in range(warmup + reps):
        d.profile(True)
        d.sweep(0, src, ds.W_MIN, ds.W_MAX, D, radius, 40)
        d.filter(0, src, 0.01, 1)
        p = d.get_profile()
        if i >= warmup:
            sweep.append(p["k_plane_sweep"][0]), filt.append(p["k_depth_filter_points"][0])
    f = d.depth(0, filtered=True)
    one = sc.one_plane(w, h)
    inputs = [("a_filtered_map", f["depth"], f["plane"], 4, 1), ("b_one_plane", sc.depth_map(one), one, 4, 1),
              ("c_serpentine", sc.depth_map(sc.serpentine(w, h)), sc.serpentine(w, h), 4, 1),
              ("d_checkerboard", sc.depth_map(sc.checkerboard(w, h)), sc.checkerboard(w, h), 4, 0)]
    row = {"case": name, "width": w, "height": h, "planes": D, "radius": radius, "sources": n_src, "reps": reps, "warmup": warmup,
           "k_plane_sweep": stats(sweep), "k_depth_filter_points": stats(filt), "inputs": {}}
    for key, depth, plane, min_size, max_diff in inputs:
        per = {k: [] for k in d.get_speckle_profile()}
        kept = 0
        for i in range(warmup + reps):
            d.profile(True)
            out = d.speckle_maps(depth, plane, min_size, max_diff)
            p = d.get_speckle_profile()
            assert [v[1] for v in p.values()] == [1, 1, 1, 1], p
            kept = int((out["plane"] >= 0).sum())
            if i >= warmup:
                for k in per:
                    per[k].append(p[k][0])
        total = [sum(per[k][i] for k in per) for i in range(reps)]
        row["inputs"][key] = {"min_size": min_size, "max_diff": max_diff, "valid": int((plane >= 0).sum()), "kept": kept,
                              "segments": int((out["label"].reshape(-1) == np.arange(w * h)).sum()),
                              "four_launches": stats(total), **{k: stats(per[k]) for k in per}}
    d.profile(False)
    d.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run("640x480 D=128 r=2 V=4", 640, 480, 128, 2, 4, a.reps, a.warmup),
            run("320x240 D=64 r=2 V=2", 320, 240, 64, 2, 2, a.reps, a.warmup)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/speckle_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
