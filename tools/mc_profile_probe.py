#!/usr/bin/env python3
"""What the first-collision profile (POCS_OPT_MC_WAYPOINT_COUNTS) and the MC stop (POCS_OPT_MC_RISK_BOUND) cost and save a
per-step Monte-Carlo call on the GPU.

Cases (per-step launch form, POCS_OPT_MC_FUSED = 0, --particles each, default 10^6):
  cand8     the 8 candidate plans of tests/test_plan_risk_bound.py (lengths 20, 56, 1, 33, 2, 56', 7, 120) as one call of plans
  batch20   set_batch(20) on the bundled plan (56 waypoints)
Modes:
  off       both options 0: today's kernels.  Run it with POCS_LIB set to another commit's library for the other side of an
            A/B (such a library needs neither option: none is set in this mode)
  counts    POCS_OPT_MC_WAYPOINT_COUNTS = 1
  stop      cand8 only: POCS_OPT_MC_RISK_BOUND = 1 under --bound (default 0.2), with the E[p] the call reported and
            `removed` = 1 - sum (E[p] - 1) / sum (W[p] - 1), the share of the (plan, step) launches' work that the stop took away

GPU time per call = the replayed graph's span between one pair of events (POCS_OPT_PROFILE = 2), median of the repeats.
A stopped plan's blocks are still launched and return in their head.  One JSON line per (case, mode).

  python tools/mc_profile_probe.py [--reps 10] [--warm 3] [--modes off,counts,stop] [--only cand8] [--bound 0.2]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import pocs_amd  # noqa: E402

K, SEED = 1, 0x5EED0001
LENGTHS = (20, 56, 1, 33, 2, 56, 7, 120)


def prefix(plan, W):
    return dict(traj=np.asarray(plan["traj"])[:W].copy(), odom=np.asarray(plan["odom"])[:W - 1].copy().reshape(-1, 3))


def shifted(plan, dy):
    traj = np.asarray(plan["traj"]) + np.array([0.0, dy, 0.0])
    return dict(traj=traj, odom=pocs_amd.planio.path_odometry(traj))


def candidates(plan):
    out, seen56 = [], False
    for W in LENGTHS:
        if W == 56 and seen56:
            out.append(shifted(plan, 0.1))
        elif W <= 56 and W != 33:
            out.append(prefix(plan, W))
        else:
            out.append(pocs_amd.resample_plan(plan, W))
        seen56 = seen56 or W == 56
    return out


def run_case(name, mode, bound, N, plan, env, reps, warm):
    with pocs_amd.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        if name == "cand8":
            c.set_plans(candidates(plan))
            lengths = list(LENGTHS)
        else:
            c.set_batch(20)
            lengths = [len(plan["traj"])] * 20
        c.set_option(pocs_amd.OPT_MC_FUSED, 0)
        if mode == "counts":
            c.set_option(pocs_amd.OPT_MC_WAYPOINT_COUNTS, 1)
        if mode == "stop":
            c.set_plan_risk_bound(bound)
            c.set_option(pocs_amd.OPT_MC_RISK_BOUND, 1)
        c.set_option(pocs_amd.OPT_PROFILE, 2)
        for _ in range(warm):
            c.run_simulation()
        ms = []
        for _ in range(reps):
            c.set_seed(SEED)                                 # the same particles every repeat: a stop at the same waypoints
            c.run_simulation()
            ms.append(c.kernel_time()[0])
        E = c.plan_evaluated().tolist() if mode == "stop" else lengths
        counts = c.mc_batch_counts()
    steps = sum(w - 1 for w in lengths)
    return dict(case=name, mode=mode, bound=bound if mode == "stop" else None, runs=len(lengths), waypoints=sum(lengths), N=N,
                gpu_ms_median=round(statistics.median(ms), 4), gpu_ms_min=round(min(ms), 4), gpu_ms_max=round(max(ms), 4),
                reps=reps, evaluated=E, removed=round(1.0 - sum(e - 1 for e in E) / steps, 4), counts=counts)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--modes", default="off,counts,stop")
    ap.add_argument("--only", choices=["cand8", "batch20"])
    ap.add_argument("--bound", type=float, default=0.2)
    ap.add_argument("--particles", type=int, default=1_000_000)
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    for name in ([args.only] if args.only else ["cand8", "batch20"]):
        for mode in args.modes.split(","):
            if mode == "stop" and name != "cand8":
                continue                                     # the bound acts on calls of plans only
            r = run_case(name, mode, args.bound, args.particles, plan, env, args.reps, args.warm)
            print("%-8s %-6s %3d runs, %4d waypoints, N %d: %8.3f ms per call (GPU, median of %d; %.3f .. %.3f)%s"
                  % (name, mode, r["runs"], r["waypoints"], r["N"], r["gpu_ms_median"], r["reps"], r["gpu_ms_min"], r["gpu_ms_max"],
                     "  removed %.3f  E %s" % (r["removed"], r["evaluated"]) if mode == "stop" else ""), file=sys.stderr)
            print(json.dumps(r))


if __name__ == "__main__":
    main()
