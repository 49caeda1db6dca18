#!/usr/bin/env python3
"""What a risk bound (pocs_set_plan_risk_bound) saves a call of candidate plans on the GPU.

Cases (10^6 samples, K = 3, timed as tools/plan_batch_probe.py times its cases):
  uniform20, mixed20   that tool's cases, bound off: what this build's bound-off call costs (run it with POCS_LIB set to
                       another commit's library for the other side of an A/B; such a library needs no risk bound)
  shift20              20 laterally shifted copies of the bundled plan (56 waypoints each, dy = 0.01 p for plan p):
                       bound off, then one case per --bound (default 0.2 and 0.05) with the E[p] the call reported

GPU time per call = the replayed graph's span between one pair of events (POCS_OPT_PROFILE = 2), median of the
repeats.  `share` = sum E[p] / sum W[p], the part of the work that was left; the expectation is a time between that share
and 1 of the bound-off time -- a stopped plan's blocks are still launched and cost one memory round trip each, and the
launches of the plans left no longer fill the chip.  One JSON line per case.

  python tools/plan_risk_probe.py [--reps 10] [--warm 3] [--only shift20] [--bound 0.2 --bound 0.05]
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


def shifted(plan, dy):
    traj = np.asarray(plan["traj"]) + np.array([0.0, dy, 0.0])
    return dict(traj=traj, odom=pocs_amd.planio.path_odometry(traj))


def mixed_lengths(n=20, lo=4, hi=56):
    Ws = [int(round(x)) for x in np.linspace(lo, hi, n)]
    return [Ws[(7 * i) % n] for i in range(n)]          # tools/plan_batch_probe.py's scrambled order


def plans_of(name, plan):
    if name == "uniform20":
        return [plan] * 20
    if name == "mixed20":
        return [prefix(plan, W) for W in mixed_lengths()]
    return [shifted(plan, 0.01 * p) for p in range(20)]


def run_case(name, bound, plan, env, reps, warm):
    plans = plans_of(name, plan)
    lengths = [len(pl["traj"]) for pl in plans]
    with pocs_amd.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_plans(plans)
        if bound < 1.0:
            c.set_plan_risk_bound(bound)
        c.set_option(pocs_amd.OPT_PROFILE, 2)
        for _ in range(warm):
            c.run_gmm_estimation()
        ms, shares = [], []
        for _ in range(reps):
            c.run_gmm_estimation()
            ms.append(c.kernel_time()[0])
            E = c.plan_evaluated().tolist() if bound < 1.0 else lengths
            shares.append(sum(E) / sum(lengths))
        finals = c.batch_probabilities()
    med = statistics.median(ms)
    return dict(case=name, bound=bound, plans=len(plans), waypoints=sum(lengths), N=N, K=K,
                gpu_ms_median=round(med, 4), gpu_ms_min=round(min(ms), 4), gpu_ms_max=round(max(ms), 4), reps=reps,
                evaluated_last_call=E, share_median=round(statistics.median(shares), 4),
                share_min=round(min(shares), 4), share_max=round(max(shares), 4),
                probabilities_last_call=[round(float(x), 6) for x in finals])


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--only", choices=["uniform20", "mixed20", "shift20"])
    ap.add_argument("--bound", type=float, action="append", help="risk bounds of the shift20 cases (default 0.2 and 0.05)")
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    names = [args.only] if args.only else ["uniform20", "mixed20", "shift20"]
    cases = [(n, 1.0) for n in names] + [("shift20", b) for b in (args.bound or [0.2, 0.05]) if "shift20" in names]
    off = {}
    for name, bound in cases:
        r = run_case(name, bound, plan, env, args.reps, args.warm)
        if bound >= 1.0:
            off[name] = r["gpu_ms_median"]
        else:
            r["time_over_bound_off"] = round(r["gpu_ms_median"] / off[name], 4)
        print("%-10s bound %-5s %3d plans, %4d waypoints: %8.3f ms per call (GPU, median of %d; %.3f .. %.3f)  share evaluated %.3f%s"
              % (name, "off" if bound >= 1.0 else "%g" % bound, r["plans"], r["waypoints"], r["gpu_ms_median"], r["reps"],
                 r["gpu_ms_min"], r["gpu_ms_max"], r["share_median"],
                 "" if bound >= 1.0 else "  time / bound-off %.3f  E %s" % (r["time_over_bound_off"], r["evaluated_last_call"])),
              file=sys.stderr)
        print(json.dumps(r))


if __name__ == "__main__":
    main()
