"""Timing of the raw-frame ingest (ekf_set_frame_raw, k_frame_ingest, the raw key-frame slots) at the two
cameras of the reference: conf_sim.cfg's 2560 x 1920 x 3 at scale 10 and the kinect's 640 x 480 x 3 at scale 2.  Per geometry:
HIP-event time of the upload and of the kernel (ekf_profile_*: frame_upload, frame_ingest), the host wall clock of the whole
ekf_set_frame_raw call, of the same call from a device pointer (+ ekf_synchronize), of the route before there was an ingest
(the numpy oracle's host resize + grey, then ekf_set_frame), and of an emitting ekf_keyframe_observe with and without the
raw slots.  Medians over --reps calls after a warm-up.
Usage: python tools/frame_ingest_timing.py [--reps 200] [--out profiles/frame_ingest_mi355x.json]"""
import argparse, json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "oracle"), os.path.join(R, "tests")]
from __graft_entry__ import load_package
import frame_ingest_oracle as fi

pkg = load_package()
HBM_PEAK_GBS = 8000.0                                   # MI355X data sheet: 8 TB/s


def med_ms(fn, reps, sync=None):
    out = []
    for _ in range(reps):
        if sync:
            sync()
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return float(np.median(out) * 1e3)


def events(f, fn, reps):
    """Mean HIP-event time per call of the two launch groups."""
    f.set_option(2, 2)                                  # EKF_OPT_PROFILE = 2: events around every timed launch group
    f.profile_reset()
    for _ in range(reps):
        fn()
    f.synchronize()
    prof = f.profile()
    f.set_option(2, 0)
    return {k: prof.get(k, (0.0, 0))[0] / max(prof.get(k, (0.0, 1))[1], 1) for k in ("frame_upload", "frame_ingest")}


def observe_ms(f, sel, reps):
    """An observe that emits (EMIT_FIRST: the pose jumps, id < 5): the snapshot launches really copy."""
    def step(k=[0]):
        k[0] ^= 1
        f.setStateSegment(0, np.array([10.0 * k[0], 0, 0, 1, 0, 0, 0], f.dtype))
        f.synchronize()
        t0 = time.perf_counter()
        r = sel.observe(2)
        dt = time.perf_counter() - t0
        assert r.action == 4, r.action_name
        return dt
    for _ in range(10):
        step()
    return float(np.median([step() for _ in range(reps)]) * 1e3)


def run(name, cfg, W, H, C, reps):
    import torch
    s = cfg["scale"]
    raw = np.random.default_rng(3).integers(0, 256, size=(H, W, C)).astype(np.uint8)
    f = pkg.VSlamFilter(cfg, capacity_features=16)
    want = fi.ingest(raw, s)
    f.setFrameRaw(raw)
    assert np.array_equal(f.getFrame(), want)
    for _ in range(20):
        f.setFrameRaw(raw)
    ev_host = events(f, lambda: f.setFrameRaw(raw), reps)
    wall_host = med_ms(lambda: f.setFrameRaw(raw), reps, f.synchronize)
    t = torch.from_numpy(raw).cuda()
    torch.cuda.synchronize()
    dev = lambda: (f.setFrameRaw(t), f.synchronize())
    for _ in range(20):
        dev()
    assert np.array_equal(f.getFrame(), want)
    ev_dev = events(f, dev, reps)
    wall_dev = med_ms(dev, reps, f.synchronize)
    # the route before: resize + grey on the host (the numpy oracle), then ekf_set_frame
    slow = max(reps // 10, 5)
    host_ms = med_ms(lambda: fi.ingest(raw, s), slow)
    set_ms = med_ms(lambda: f.setFrame(want), reps, f.synchronize)
    # key frames: an emitting observe on a plain and on a raw selector, the raw frame resident
    f.setFrameRaw(raw)
    plain, rsel = pkg.KeyframeSelector(f), pkg.KeyframeSelector(f, raw_shape=raw.shape)
    obs_plain, obs_raw = observe_ms(f, plain, reps), observe_ms(f, rsel, reps)
    assert np.array_equal(rsel.emitted_raw_image(), raw)
    for h in (plain, rsel, f):
        h.close()
    mode = fi.mode(W, H, s)
    out_px = (W // s) * (H // s)
    moved = out_px * (1 + 4 * C + 32) if mode == "linear" else W * H * C + out_px      # taps + two 16-byte table records, or every byte
    kern = ev_host["frame_ingest"]
    return {"camera": name, "raw": [W, H, C], "scale": s, "path": mode, "reps": reps,
            "upload_ms": ev_host["frame_upload"], "kernel_ms": kern, "kernel_bytes": moved,
            "kernel_GBs": moved / (kern * 1e-3) / 1e9 if kern > 0 else None,
            "kernel_fraction_of_hbm_peak": moved / (kern * 1e-3) / 1e9 / HBM_PEAK_GBS if kern > 0 else None,
            "set_frame_raw_wall_ms": wall_host,
            "device_pointer": {"copy_ms": ev_dev["frame_upload"], "kernel_ms": ev_dev["frame_ingest"],
                               "wall_with_synchronize_ms": wall_dev},
            "before": {"host_resize_gray_numpy_ms": host_ms, "set_frame_wall_ms": set_ms, "sum_ms": host_ms + set_ms},
            "observe_emit_wall_ms": {"plain": obs_plain, "raw": obs_raw, "extra": obs_raw - obs_plain}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = [run("conf_sim 2560x1920x3 s=10", dict(pkg.sim_config()), 2560, 1920, 3, a.reps),
            run("kinect 640x480x3 s=2", dict(pkg.kinect_config()), 640, 480, 3, a.reps)]
    for r in rows:
        print(json.dumps(r))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump({"tool": "tools/frame_ingest_timing.py", "hbm_peak_GBs": HBM_PEAK_GBS, "results": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
