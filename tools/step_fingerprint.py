"""Fingerprint of the update's launch schedule, for comparing two commits: for a fixed list of cases -- one per branch of
the schedule, at the smallest shape that reaches it -- three predict / update frames of the synthetic stream on a fresh
filter, then ONE line: the case, its launch_counts() and the SHA-256 of getFullState() and getFullSigma() (the step is
reproducible to the bit, profiles/r5_determinism_probe.txt).  Run it on both commits and diff the outputs; the hashes
belong to one compiler and are no golden values.
usage: python3 tools/step_fingerprint.py"""
import hashlib, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from __graft_entry__ import load_package
pkg = load_package()
from ekf_monoslam_amd import synthetic
FRAMES = 3
F32, F64 = np.float32, np.float64
W0, W1 = {"EKF_W_RECOMPUTE": "0"}, {"EKF_W_RECOMPUTE": "1"}
NOSPLIT = {"EKF_SPLIT_BF16": "0"}
FORCED = {"EKF_SHARD_FORCE_COLLECTIVE": "1"}
# (name, dtype, N, plane rows, environment knobs, MFMA option, what else: "gain" / "sharded")
CASES = [
    ("f32 N=8 plane (one-launch update)", F32, 8, True, {}, 1, ""),
    ("f32 N=32 plane (one-launch update)", F32, 32, True, {}, 1, ""),
    ("f32 N=40 plane (one block, all-in-one)", F32, 40, True, {}, 1, ""),
    ("f32 N=200 (one chunk, fused block step)", F32, 200, False, {}, 1, ""),
    ("f32 N=640 defaults (bf16x6, row rider, state-update tail)", F32, 640, False, {}, 1, ""),
    ("f32 N=640 split=0 wrec=0 fuse_wu=0", F32, 640, False, {**NOSPLIT, **W0, "EKF_FUSE_WU": "0"}, 1, ""),
    ("f32 N=640 split=0 wrec=0 fuse_wu=2", F32, 640, False, {**NOSPLIT, **W0, "EKF_FUSE_WU": "2"}, 1, ""),
    ("f32 N=640 split=0 wrec=1 fuse_wu=0", F32, 640, False, {**NOSPLIT, **W1, "EKF_FUSE_WU": "0"}, 1, ""),
    ("f32 N=640 split=0 wrec=1 fuse_wu=2", F32, 640, False, {**NOSPLIT, **W1, "EKF_FUSE_WU": "2"}, 1, ""),
    ("f32 N=640 chain_fused_diag=0", F32, 640, False, {"EKF_CHAIN_FUSED_DIAG": "0"}, 1, ""),
    ("f64 N=40", F64, 40, False, {}, 1, ""),
    ("f64 N=200", F64, 200, False, {}, 1, ""),
    ("f32 N=200 VALU tiles", F32, 200, False, {}, 0, ""),
    ("f64 N=200 VALU tiles", F64, 200, False, {}, 0, ""),
    ("f32 N=200 gain", F32, 200, False, {}, 1, "gain"),
    ("f32 N=640 sharded world 1, forced collective, wrec=0", F32, 640, False, {**FORCED, **W0}, 1, "sharded"),
    ("f32 N=640 sharded world 1, forced collective, wrec=1", F32, 640, False, {**FORCED, **W1}, 1, "sharded"),
    ("f32 N=640 sharded world 1, forced collective, distributed chain", F32, 640, False,
     {**FORCED, "EKF_SHARD_DIST_MIN_BLOCKS": "2"}, 1, "sharded"),
]
cfg = pkg.kinect_config()
streams = {}


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:32]


def one(name, dtype, n_feat, plane, env, mfma, extra):
    if n_feat not in streams:
        streams[n_feat] = synthetic.measurement_stream(cfg, n_feat, FRAMES, sigma_px=0.5)
    px0, z = streams[n_feat]
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)                                   # the knobs are read when the filter is created / configured
    try:
        f = pkg.VSlamFilter(cfg, capacity_features=n_feat + 8, dtype=dtype)
        f.set_option(1, mfma)                                # EKF_OPT_USE_MFMA
        f.setDt(1 / 30.0)
        for (u, v) in px0:
            assert f.addFeature((u, v)) == 1
        note = ""
        if extra == "sharded":
            import torch
            import torch.distributed as dist
            from ekf_monoslam_amd import sharded
            if not dist.is_initialized():
                os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
                os.environ.setdefault("MASTER_PORT", "29541")
                dist.init_process_group("gloo", rank=0, world_size=1)
            sharded.configure(f, 0, 1)
            d_z = torch.from_numpy(np.ascontiguousarray(z.reshape(FRAMES, -1), dtype)).cuda()
            idx = np.arange(n_feat, dtype=np.int32)
            for k in range(FRAMES):
                f.predict()
                sharded.shard_update(f, d_z[k].data_ptr(), idx, plane)
            if "EKF_SHARD_DIST_MIN_BLOCKS" in env and f.launch_counts().get("chain_dist_gather", 0) == 0:
                note = " | the distributed chain did NOT run at world 1"
        else:
            for k in range(FRAMES):
                f.predict()
                h, vis, rem, _ = f.predictions()
                sel = np.nonzero(vis.astype(bool))[0].astype(np.int32)
                f.update(z[k][sel].reshape(-1).astype(dtype), sel, plane_constraint=plane)
        f.synchronize()
        line = f"{name} | {json.dumps(f.launch_counts(), sort_keys=True)} | mu {sha(f.getFullState())} | Sigma {sha(f.getFullSigma())}"
        if extra == "gain":
            line += f" | gain {sha(f.getGain())}"
        print(line + note, flush=True)
        f.close()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


for case in CASES:
    one(*case)
