"""Host-visible latency of the key-frame selector against the getter sequence it replaces, at a 32-feature fp32 map, in
one session: python tools/keyframe_latency.py [--out profiles/keyframe_latency_mi355x.json]

  observe_idle        KeyframeSelector.observe() on a frame that stores and emits nothing (no frame set: one launch)
  observe_idle_frame  the same with a 640x480 frame set (the image launch returns at once)
  observe_candidate   observe() that stores a candidate: the probe plus the 640x480 device-to-device snapshot
  getters             getState + getSigmaBlock(0, 0, 7, 7) + Covariance_Parameter: three round trips

1000 calls each, every call timed on its own with a host clock (each ends in a stream synchronisation); median and p95."""
import json, os, sys, time
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R]
from __graft_entry__ import load_package
pkg = load_package()
from ekf_monoslam_amd import synthetic
N, REPS = 32, 1000
out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
cfg = dict(pkg.kinect_config())
px0, z = synthetic.measurement_stream(cfg, N, 20, sigma_px=0.5)


def make_filter(config):
    f = pkg.VSlamFilter(config, capacity_features=N + 8)
    f.setDt(1 / 30.0)
    for (u, v) in px0:
        assert f.addFeature((u, v)) == 1
    idx = np.arange(N, dtype=np.int32)
    for k in range(5):
        f.predict(); f.update(z[k].reshape(-1).astype(np.float32), idx)
    f.synchronize()
    return f


def series(fn, before=None):
    for _ in range(50):
        if before: before()
        fn()
    t = np.zeros(REPS)
    for i in range(REPS):
        if before: before()
        t0 = time.perf_counter()
        fn()
        t[i] = time.perf_counter() - t0
    return {"median_us": float(np.median(t) * 1e6), "p95_us": float(np.percentile(t, 95) * 1e6)}


res = {"features": N, "dtype": "float32", "calls": REPS}
f = make_filter(cfg)
res["getters"] = series(lambda: (f.getState(), f.getSigmaBlock(0, 0, 7, 7), f.Covariance_Parameter()))
for name, fn in (("getState", f.getState), ("getSigmaBlock_7x7", lambda: f.getSigmaBlock(0, 0, 7, 7)),
                 ("Covariance_Parameter", f.Covariance_Parameter)):
    res[name] = series(fn)
sel = pkg.KeyframeSelector(f, 1e6)                       # nothing ever reaches half of this threshold
counter = [0]
def idle():
    counter[0] += 1
    r = sel.observe(counter[0] + 10)
    assert r.action == 0
res["observe_idle"] = series(idle)
sel.close(); f.close()

big = dict(cfg, image_width=640, image_height=480)
f = make_filter(big)
f.setFrame((np.arange(640 * 480) % 251).astype(np.uint8).reshape(480, 640))
sel = pkg.KeyframeSelector(f, 1e6)
res["observe_idle_frame"] = series(idle)
sel.close()
# every observe stores a candidate: the state sits inside the window of a fresh selector state (reset, not timed)
mu = f.getFullState()
sel = pkg.KeyframeSelector(f, 1000.0)
mu[:3] = [200.0, 0, 0]                                   # D = 666 + rotation: inside (500, 1000)
f.setFullState(mu)
def cand():
    counter[0] += 1
    r = sel.observe(counter[0] + 10)
    assert r.action == 1, r
res["observe_candidate_640x480"] = series(cand, before=sel.reset)
sel.close(); f.close()
res["observe_not_above_getters"] = res["observe_idle"]["median_us"] <= res["getters"]["median_us"]
print(json.dumps(res, indent=1))
if out_path:
    json.dump(res, open(out_path, "w"), indent=1)
