"""Timing of the on-demand rectification launch (k_frame_rectify behind ekf_get_frame_rectified) at the matcher
frame of the real-camera configs, 640 x 480 x 1, and at the simulator's raw frame, 2560 x 1920 x 3 at scale 10, both with
the firewire lens (conf_firewire.cfg) so that the taps are really displaced.  Per geometry: the mean HIP-event time of the
launch over --reps calls (ekf_profile_*: frame_rectify), and as the yardstick the mean event time of a device-to-device
copy of the same number of output bytes in the same session.  There is no gate: the launch runs once per key frame.
Usage: python tools/rectify_timing.py [--reps 200] [--out profiles/rectify_timing_mi355x.json]"""
import argparse, json, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "oracle"), os.path.join(R, "tests")]
from __graft_entry__ import load_package
import rectify_oracle as ro

pkg = load_package()
FIREWIRE = dict(k1=-0.45720, k2=0.30980, k3=-0.13950, p1=-0.00265, p2=0.00078)


def kernel_ms(f, fn, reps):
    f.set_option(2, 2)                                  # EKF_OPT_PROFILE = 2: events around every timed launch group
    f.profile_reset()
    for _ in range(reps):
        fn()
    f.synchronize()
    ms, n = f.profile().get("frame_rectify", (0.0, 0))
    f.set_option(2, 0)
    assert n == reps, (n, reps)
    return ms / n


def copy_ms(nbytes, reps):
    import torch
    src = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(20):
        dst.copy_(src)
    torch.cuda.synchronize()
    tot = 0.0
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        tot += a.elapsed_time(b)
    return tot / reps


def run(name, cfg, raw, frame, reps):
    f = pkg.VSlamFilter(cfg, capacity_features=16)
    if raw:
        f.setFrameRaw(frame)
    else:
        f.setFrame(frame)
    get = lambda: f.getFrameRectified(raw=raw)
    L = ro.lens(cfg)
    assert np.array_equal(get(), ro.rectify_image(frame, L, cfg["scale"] if raw else 1)), "device image differs from the oracle"
    for _ in range(20):
        get()
    k_ms = kernel_ms(f, get, reps)
    f.close()
    c_ms = copy_ms(frame.nbytes, reps)
    return {"case": name, "shape": list(frame.shape), "output_bytes": int(frame.nbytes), "reps": reps,
            "k_frame_rectify_ms": k_ms, "device_copy_same_bytes_ms": c_ms, "ratio_kernel_over_copy": k_ms / c_ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rng = np.random.default_rng(3)
    kin = dict(pkg.kinect_config(), scale=1, image_width=640, image_height=480, fx=563.21765, fy=558.45293, u0=347.75115,
               v0=246.19144, **FIREWIRE)
    sim = dict(pkg.sim_config(), **FIREWIRE)
    s = int(sim["scale"])
    W, H = int(sim["image_width"]) * s, int(sim["image_height"]) * s
    rows = [run("matcher frame 640x480x1", kin, False, rng.integers(0, 256, size=(480, 640)).astype(np.uint8), a.reps),
            run("raw frame %dx%dx3 s=%d" % (W, H, s), sim, True, rng.integers(0, 256, size=(H, W, 3)).astype(np.uint8), a.reps)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/rectify_timing.py", "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
