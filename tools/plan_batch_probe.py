#!/usr/bin/env python3
"""What a batch of candidate plans (pocs_set_plans) costs on the GPU, against the plain batch of runs it generalises.

Cases (10^6 samples, K = 3, the bundled plan of 56 waypoints):
  batch20    set_batch(20): 20 runs of the bundled plan per call
  uniform20  a plan batch of 20 copies of the bundled plan          -- expected within noise of batch20
  mixed20    20 plans of mixed lengths (prefixes of the bundled plan, 4 .. 56 waypoints, in scrambled order)
             -- the launch of waypoint w covers only the plans longer than w, so this should take clearly less
             time than 20 full-length plans

GPU time per call = the replayed graph's span between one pair of events (POCS_OPT_PROFILE = 2), median of the
repeats; evaluations = N x (sum of the plans' lengths).  One JSON line per case.

  python tools/plan_batch_probe.py [--reps 10] [--only mixed20]
Under rocprofv3 --kernel-trace --stats, `--only mixed20` gives the mixed batch's launches alone.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import pocs_amd  # noqa: E402

N, K, SEED = 1_000_000, 3, 0x5EED0001


def prefix(plan, W):
    return dict(traj=np.asarray(plan["traj"])[:W].copy(), odom=np.asarray(plan["odom"])[:W - 1].copy().reshape(-1, 3))


def mixed_lengths(n=20, lo=4, hi=56):
    Ws = [int(round(x)) for x in np.linspace(lo, hi, n)]
    return [Ws[(7 * i) % n] for i in range(n)]          # a scrambled order (7 is prime to 20)


def run_case(name, plan, env, reps, warm):
    with pocs_amd.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        if name == "batch20":
            c.set_batch(20)
            lengths = [len(plan["traj"])] * 20
        elif name == "uniform20":
            c.set_plans([plan] * 20)
            lengths = [len(plan["traj"])] * 20
        else:
            lengths = mixed_lengths()
            c.set_plans([prefix(plan, W) for W in lengths])
        c.set_option(pocs_amd.OPT_PROFILE, 2)
        for _ in range(warm):
            c.run_gmm_estimation()
        ms = []
        for _ in range(reps):
            c.run_gmm_estimation()
            ms.append(c.kernel_time()[0])
        finals = c.batch_probabilities()
    evals = N * sum(lengths)
    med = statistics.median(ms)
    return dict(case=name, plans=len(lengths), waypoints=sum(lengths), max_W=max(lengths), N=N, K=K,
                gpu_ms_median=round(med, 4), gpu_ms_min=round(min(ms), 4), gpu_ms_max=round(max(ms), 4), reps=reps,
                evals_per_s=evals / (med * 1e-3), first_probabilities=[float(x) for x in finals[:3]])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--only", choices=["batch20", "uniform20", "mixed20"])
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    cases = [args.only] if args.only else ["batch20", "uniform20", "mixed20"]
    for name in cases:
        r = run_case(name, plan, env, args.reps, args.warm)
        print("%-10s %3d plans, %4d waypoints: %8.3f ms per call (GPU, median of %d; %.3f .. %.3f), %.3e evals/s"
              % (name, r["plans"], r["waypoints"], r["gpu_ms_median"], r["reps"], r["gpu_ms_min"], r["gpu_ms_max"], r["evals_per_s"]),
              file=sys.stderr)
        print(json.dumps(r))


if __name__ == "__main__":
    main()
