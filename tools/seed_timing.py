"""Timing of ekf_find_new_features (the device corner detector, csrc/ekf_features.hpp) at 320 x 240 (kinect config)
and 640 x 480 (the default config): HIP-event time of each of the detector's launch groups (ekf_profile_*:
seed_mask, seed_response, seed_candidates, seed_select) and the host wall clock of the whole call (mask upload, five launches, one read-back of the corners).
Usage: python tools/seed_timing.py [--out profiles/seed_timing_mi355x.json]"""
import argparse, json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "oracle")]
from __graft_entry__ import load_package
import image_oracle as io_

pkg = load_package()
LAUNCHES = ("seed_mask", "seed_response", "seed_candidates", "seed_select")      # kernel ids of ekf_find_new_features


def run(name, cfg, num, reps=200):
    H, W = cfg["image_height"], cfg["image_width"]
    f = pkg.VSlamFilter(cfg, capacity_features=64)
    f.setFrame(io_.random_texture(H, W, seed=5))
    for _ in range(20):
        f.findNewFeatures(num, add=False)
    f.set_option(2, 2)                                  # EKF_OPT_PROFILE = 2: HIP events around every timed launch group
    f.profile_reset()
    for _ in range(reps):
        uv = f.findNewFeatures(num, add=False)
    prof = f.profile()
    f.set_option(2, 0)
    wall = []
    for _ in range(reps):
        f.synchronize()
        t0 = time.perf_counter()
        f.findNewFeatures(num, add=False)
        wall.append(time.perf_counter() - t0)
    launches = {k: prof.get(k, (0.0, 0))[0] / reps for k in LAUNCHES}
    f.close()
    w = np.sort(np.asarray(wall)) * 1e3
    return {"config": name, "width": W, "height": H, "num": num, "corners": int(len(uv)), "reps": reps,
            "device_ms_per_call": sum(launches.values()), "launch_ms_per_call": launches,
            "wall_ms_median": float(np.median(w)),
            "wall_ms_p10": float(w[len(w) // 10]), "wall_ms_p90": float(w[9 * len(w) // 10])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    kin = dict(pkg.kinect_config())
    dflt = dict(kin, image_width=640, image_height=480, window_size=21)
    rows = [run("kinect 320x240", kin, k) for k in (10, 25, 50, 100)] + [run("640x480 w21", dflt, k) for k in (10, 50)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/seed_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
