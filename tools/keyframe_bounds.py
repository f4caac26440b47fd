"""Measures the selector's deviation from the numpy oracle over the scenes of tests/keyframe_scene.py (fp32 and fp64
filters) on the GPU and writes tests/golden/keyframe_bounds.json: the measured maxima, the 10 x bounds of
tests/test_gpu_keyframes.py and the 100 x margins of tests/test_oracle_keyframes.py.
python tools/keyframe_bounds.py [--out FILE]"""
import json, os, sys
import numpy as np
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [R, os.path.join(R, "tests"), os.path.join(R, "oracle")]
from __graft_entry__ import load_package
pkg = load_package()
import keyframe_gpu_common as kc
import keyframe_scene as ks

out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else kc.BOUNDS
worst = {"D": 0.0, "c": 0.0, "pose": 0.0, "sigma": 0.0, "vrot": 0.0}
per_scene = {}
for name in sorted(ks.SCENES):
    frames = ks.SCENES[name]()
    for dt in (np.float32, np.float64):
        dev, ref, w, sel, g = kc.run_scripted(pkg, frames, dt, images=True)
        wrong = [k for k, ((r, _), o) in enumerate(zip(dev, ref)) if r.action != o["action"]]
        assert not wrong, (name, dt, wrong)
        per_scene["%s/%s" % (name, np.dtype(dt).name)] = w
        worst = {k: max(worst[k], w[k]) for k in worst}
        sel.close(); g.close()
res = {"measured": worst, "bound": {k: 10 * v for k, v in worst.items()},
       "margin": {"D": 100 * worst["D"], "c": 100 * worst["c"]}, "per_scene": per_scene,
       "note": "max |device - oracle| over tests/keyframe_scene.py on one MI355X (tools/keyframe_bounds.py): D and c per frame, "
               "pose and the 7 x 7 block per emitted record, last_vrot (radians) after every emit; bound = 10 x, margin = 100 x"}
print(json.dumps(res, indent=1))
json.dump(res, open(out, "w"), indent=1)
