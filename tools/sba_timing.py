"""HIP-event times of the GPU bundle adjustment per phase and per LM iteration, at the four test
sizes of tests/test_gpu_sba.py, with the numpy oracle's host time for the same run next to each.

    python tools/sba_timing.py [--out profiles/sba_timing_mi355x.json] [--niter 10] [--huber H] [--solver cholesky|pcg]

--huber H sets the pseudo-Huber width (pixels) on the GPU handle; the oracle column is then the robust
oracle's.  0 (the default) is the plain squared error.

Phases (ekf_sba_get_profile): prep (node matrices), Schur (per-point Jacobians, Hpp^-1, tp, T_a), assemble (B, the
6 x 6 blocks of A, the diagonal, the copy for the refinement), factor + solve (Cholesky, two triangular solves, the
residual, the refinement), update + cost.  The first run of each size is a warm-up (module load, allocation).

--solver pcg times the block-Jacobi PCG solver with the default CG settings and writes
profiles/sba_pcg_timing_mi355x.json: the "factor + solve" phase is then the block inverse and the CG, and each row also
holds the CG iterations per solve, the solve time per LM iteration spread over the CG rounds enqueued (cg_max_iters) and
over the CG iterations actually made, and the device memory the handle took.  The oracle column is the PCG oracle's.
--big adds a 1023-free-node scene (the Cholesky solver's limit), GPU only.
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
    ap.add_argument("--out", default=None)
    ap.add_argument("--niter", type=int, default=10)
    ap.add_argument("--huber", type=float, default=0.0)
    ap.add_argument("--solver", choices=["cholesky", "pcg"], default="cholesky")
    ap.add_argument("--big", action="store_true", help="add (1023, 27000), without the oracle")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "sba_pcg_timing_mi355x.json" if a.solver == "pcg"
                             else "sba_timing_mi355x.json")
    import torch
    pkg = g.load_package()
    rows = []
    for nfree, npts in SIZES + ([(1023, 27000)] if a.big else []):
        scene = sc.make_scene(nfree, npts, seed=nfree)
        for rep in range(2):
            free0 = torch.cuda.mem_get_info()[0]
            ba = pkg.BundleAdjuster(scene["camera"], capacity_nodes=len(scene["nodes"]),
                                    capacity_points=len(scene["points"]), capacity_projections=len(scene["node"]),
                                    solver=a.solver)
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
            cg_it = ba.cg_log()[0].tolist()
            cg_max = ba.get_cg()[1]
            mem_mb = (free0 - torch.cuda.mem_get_info()[0]) / 2.0 ** 20
            ba.close()
        if nfree > 299:                              # the numpy oracle is too slow to be worth a column here
            ref = None
        elif a.solver == "pcg":
            import sba_pcg_oracle as po
            ref = po.pcg_system(scene, a.huber if a.huber else None)
        else:
            ref = sc.oracle_system(scene)
        if a.huber and a.solver != "pcg":
            import sba_robust_oracle as ro
            ref, plain = ro.RobustSysSBA(scene["camera"], a.huber), ref
            ref.trans, ref.qrot, ref.points, ref.tracks = plain.trans, plain.qrot, plain.points, plain.tracks
            ref.valid = [{ni: True for ni in tr} for tr in ref.tracks]
        t0 = time.perf_counter()
        it_ref = ref.do_sba(a.niter, 1e-4) if ref is not None else None
        host = (time.perf_counter() - t0) * 1e3
        row = dict(free_nodes=nfree, points=npts, projections=nprj, iterations=it, oracle_iterations=it_ref,
                   gpu_run_wall_ms=round(wall, 3), gpu_phase_ms_total={k: round(float(v), 4) for k, v in zip(PHASES, ph)},
                   gpu_ms_per_iteration=[round(float(v), 4) for v in per_iter],
                   gpu_ms_per_iteration_median=round(float(np.median(per_iter)), 4) if len(per_iter) else None,
                   oracle_host_ms=round(host, 1) if ref is not None else None, solver=a.solver,
                   device_memory_mb=round(mem_mb, 1))
        if a.solver == "pcg" and it > 0:
            solve = float(ph[3]) / len(per_iter)
            row.update(cg_iterations=cg_it, cg_max_iters=cg_max, solve_ms_per_lm_iteration=round(solve, 4),
                       solve_us_per_enqueued_cg_round=round(1e3 * solve / cg_max, 3),
                       solve_us_per_cg_iteration_made=round(1e3 * solve * len(cg_it) / max(sum(cg_it), 1), 3))
        rows.append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"device": "MI355X (gfx950)", "niter": a.niter, "lambda": 1e-4, "huber": a.huber, "solver": a.solver,
                   "sizes": rows}, fh,
                  indent=1)


if __name__ == "__main__":
    main()
