#!/usr/bin/env python3
"""What evaluating a tree of candidate plans once per node (pocs_set_plan_tree) saves over evaluating its root-to-leaf
paths as a batch of plans (pocs_set_plans under common random numbers), on one context of one GPU.

Trees (10^6 samples, K = 3, no samples stored on either side):
  branches   the bundled plan with three branches at waypoint 20 and two on each at waypoint 40, plus a short plan that
             leaves the trunk at waypoint 20 (tests/test_plan_tree.py's tree): 7 leaves
  bushy      eight branches at waypoint 5, each fanning out into 24 at waypoint 50: 192 leaves, S / T > 8, eight or more
             nodes on 50 of the 56 levels

T = nodes of the tree, S = waypoints of its leaf paths added up (what the batch of plans evaluates).  GPU time per call =
the replayed graph's span between one pair of events (POCS_OPT_PROFILE = 2); the two forms ALTERNATE on the one context
(set the tree, call, clear it, set the plans, call, ...), median of the repeats.  wall = the whole library call, host
chains and -- the shape changes with every switch -- the graph's capture included.  evals/s = node (or waypoint)
evaluations x samples per GPU second.  One JSON line per tree.

  python tools/plan_tree_probe.py [--reps 10] [--warm 2] [--only bushy] [--samples 1000000]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
import pocs_amd  # noqa: E402

K, SEED = 3, 0x5EED0001


def branch(plan, j, dy):
    """`plan` with the waypoints after waypoint j shifted laterally by dy and fresh odometry from step j on."""
    t, o = np.asarray(plan["traj"]).copy(), np.asarray(plan["odom"]).copy().reshape(-1, 3)
    if dy != 0.0:
        t[j + 1:, 1] += dy
        o[j:] = pocs_amd.planio.path_odometry(t[j:])
    return dict(traj=t, odom=o)


def plans_of(name, plan):
    if name == "branches":
        out = [branch(branch(plan, 20, a), 40, b) for a in (0.0, 0.1, -0.1) for b in (0.0, 0.05)]
        t = np.asarray(plan["traj"])[:22].copy()
        t[21, 1] += 0.07
        o = np.asarray(plan["odom"])[:21].copy()
        o[20:] = pocs_amd.planio.path_odometry(t[20:])
        return out + [dict(traj=t, odom=o)]
    return [branch(branch(plan, 5, 0.01 * i), 50, 0.002 * j) for i in range(8) for j in range(24)]


def run_case(name, plan, env, N, reps, warm):
    plans = plans_of(name, plan)
    parent, poses, odoms, leaf = pocs_amd.tree_from_plans(plans)
    T, S = len(parent), sum(len(pl["traj"]) for pl in plans)
    depth = np.zeros(T, dtype=int)
    for n in range(1, T):
        depth[n] = depth[parent[n]] + 1
    widths = np.bincount(depth)
    gpu, wall = dict(tree=[], plans=[]), dict(tree=[], plans=[])
    with pocs_amd.Context(0) as c:
        c.configure(plan, env, K=K, N=N, seed=SEED)
        c.set_option(pocs_amd.OPT_PLAN_SEEDS, 1)
        c.set_option(pocs_amd.OPT_STORE_SAMPLES, 0)
        c.set_option(pocs_amd.OPT_PROFILE, 2)
        for rep in range(warm + reps):
            c.set_plan_tree(parent, poses, odoms)
            c.set_seed(SEED)
            t0 = time.perf_counter()
            c.run_gmm_estimation()
            t1 = time.perf_counter()
            tree_ms = c.kernel_time()[0]
            at_leaves = c.tree_probabilities()[leaf]
            c.clear_plan_tree()
            c.set_plans(plans)
            c.set_seed(SEED)
            t2 = time.perf_counter()
            c.run_gmm_estimation()
            t3 = time.perf_counter()
            plans_ms = c.kernel_time()[0]
            assert np.array_equal(at_leaves, c.batch_probabilities()), "the tree's leaves and their paths differ"
            c.clear_plans()
            if rep >= warm:
                gpu["tree"].append(tree_ms); gpu["plans"].append(plans_ms)
                wall["tree"].append(1e3 * (t1 - t0)); wall["plans"].append(1e3 * (t3 - t2))
    med = {k: statistics.median(v) for k, v in gpu.items()}
    return dict(tree=name, T=T, S=S, S_over_T=round(S / T, 3), leaves=len(plans), levels=len(widths),
                levels_with_8_nodes=int(np.count_nonzero(widths >= 8)), widest_level=int(widths.max()), N=N, K=K, reps=reps,
                tree_gpu_ms_median=round(med["tree"], 4), tree_gpu_ms_min=round(min(gpu["tree"]), 4), tree_gpu_ms_max=round(max(gpu["tree"]), 4),
                plans_gpu_ms_median=round(med["plans"], 4), plans_gpu_ms_min=round(min(gpu["plans"]), 4), plans_gpu_ms_max=round(max(gpu["plans"]), 4),
                plans_over_tree=round(med["plans"] / med["tree"], 3),
                tree_evals_per_s=round(T * N / (med["tree"] * 1e-3), 0), plans_evals_per_s=round(S * N / (med["plans"] * 1e-3), 0),
                tree_wall_ms_median=round(statistics.median(wall["tree"]), 3), plans_wall_ms_median=round(statistics.median(wall["plans"]), 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=2)
    ap.add_argument("--only", choices=["branches", "bushy"])
    ap.add_argument("--samples", type=int, default=1_000_000)
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    for name in ([args.only] if args.only else ["branches", "bushy"]):
        r = run_case(name, plan, env, args.samples, args.reps, args.warm)
        print("%-9s T %4d  S %5d  S/T %5.2f: tree %9.3f ms, plans %9.3f ms per call (GPU, median of %d)  plans / tree %.2f   "
              "evals/s tree %.3g, plans %.3g   wall tree %.1f ms, plans %.1f ms"
              % (name, r["T"], r["S"], r["S_over_T"], r["tree_gpu_ms_median"], r["plans_gpu_ms_median"], r["reps"], r["plans_over_tree"],
                 r["tree_evals_per_s"], r["plans_evals_per_s"], r["tree_wall_ms_median"], r["plans_wall_ms_median"]), file=sys.stderr)
        print(json.dumps(r))


if __name__ == "__main__":
    main()
