"""HIP-event times of the GPU bundle adjustment per phase and per LM iteration, at the four test
sizes of tests/test_gpu_sba.py, with the numpy oracle's host time for the same run next to each.

    python tools/sba_timing.py [--out profiles/sba_timing_mi355x.json] [--niter 10] [--huber H]

--huber H sets the pseudo-Huber width (pixels) on the GPU handle; the oracle column is then the robust
oracle's.  0 (the default) is the plain squared error.

Phases (ekf_sba_get_profile): prep (node matrices), Schur (per-point Jacobians, Hpp^-1, tp, T_a), assemble (B, the
6 x 6 blocks of A, the diagonal, the copy for the refinement), factor + solve (Cholesky, two triangular solves, the
residual, the refinement), update + cost.  The first run of each size is a warm-up (module load, allocation).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as g  # noqa: E402
import sba_scene as sc  # noqa: E402

SIZES = [(1, 40), (11, 300), (59, 2000), (299, 8000)]
PHASES = ["prep", "schur", "assemble", "factor_solve", "update_cost"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sba_timing_mi355x.json"))
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--huber", type=float, default=0.0)
    a = ap.parse_args()
    pkg = g.load_package()
    rows = []
    for nfree, npts in SIZES:
        scene = sc.make_scene(nfree, npts, seed=nfree)
        for rep in range(2):
            ba = pkg.BundleAdjuster(scene["camera"], capacity_nodes=len(scene["nodes"]),
                                    capacity_points=len(scene["points"]), capacity_projections=len(scene["node"]))
            ba.add_nodes(scene["nodes"])
            ba.add_points(scene["points"])
            ba.add_projections(scene["node"], scene["point"], scene["uv"])
            ba.huber = a.huber
            ba.profile(True)
            t0 = time.perf_counter()
            it = ba.run(a.niter, 1e-4)
            wall = (time.perf_counter() - t0) * 1e3
            ph, per_iter = ba.get_profile()
            nprj = ba.counts()[2]
            ba.close()
        ref = sc.oracle_system(scene)
        if a.huber:
            import sba_robust_oracle as ro
            ref, plain = ro.RobustSysSBA(scene["camera"], a.huber), ref
            ref.trans, ref.qrot, ref.points, ref.tracks = plain.trans, plain.qrot, plain.points, plain.tracks
            ref.valid = [{ni: True for ni in tr} for tr in ref.tracks]
        t0 = time.perf_counter()
        it_ref = ref.do_sba(a.niter, 1e-4)
        host = (time.perf_counter() - t0) * 1e3
        row = dict(free_nodes=nfree, points=npts, projections=nprj, iterations=it, oracle_iterations=it_ref,
                   gpu_run_wall_ms=round(wall, 3), gpu_phase_ms_total={k: round(float(v), 4) for k, v in zip(PHASES, ph)},
                   gpu_ms_per_iteration=[round(float(v), 4) for v in per_iter],
                   gpu_ms_per_iteration_median=round(float(np.median(per_iter)), 4) if len(per_iter) else None,
                   oracle_host_ms=round(host, 1))
        rows.append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": "MI355X (gfx950)", "niter": a.niter, "lambda": 1e-4, "huber": a.huber, "sizes": rows}, fh,
                  indent=1)


if __name__ == "__main__":
    main()
