#!/usr/bin/env python3
"""What watched regions (pocs_set_regions) cost when they are on (DESIGN.md sections 5 and 10).

Legs, one context each, ALTERNATING call by call, G = 0 against G = 1 (the goal region alone: planio.goal_region, a POINT region
of 0.05 x 0.05 at the plan's last waypoint) and G = 4 (the goal, a TOUCH doorway beside the plan's middle, two POINT zones):
  gmm   bench.py's cfg2 at 20 runs per call: the bundled 56-waypoint plan and its boxes, K = 3, 10^6 samples per run, samples
        stored (the default), the call as two sub-batches (the default at this size)
  mc    bench.py's cfg5 at 64 runs per call in the per-step form: the plan resampled to 500 waypoints, 10^5 particles per run
Timed: the wall time of one pocs_run_gmm_estimation / pocs_run_simulation call (host chains, upload, graph replay, read-back, the
table's copy included).  Median, min and max of the repeats, in ms, and the ratio to the G = 0 leg; for the legs under regions, the
share of samples / particles the last call's table counts per region.

  python tools/regions_probe.py [--reps 15] [--warm 4] [--only gmm|mc] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import pocs_amd  # noqa: E402



def regions_of(plan, G):
    """G = 0: none; 1: the goal region alone; 4: the goal, a doorway the footprint passes, and two zones along the plan."""
    t = plan["traj"]
    m = len(t) // 2
    goal = pocs_amd.planio.goal_region(plan, 0.05, 0.05)
    four = [goal, [t[m][0], t[m][1] - 0.30, 0.20, 0.02, -0.2], [t[m // 2][0], t[m // 2][1], 0.04, 0.04, 0.0], [t[-2][0] + 0.1, t[-2][1], 0.05, 0.5, 0.0]]
    return {0: ([], []), 1: ([goal], [1]), 4: (four, [1, 0, 1, 1])}[G]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["gmm", "mc"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    long_plan = pocs_amd.resample_plan(plan, 500)

    def gmm(G):
        c = pocs_amd.Context(0)
        c.configure(plan, env, K=3, N=1000000, seed=0x5EED0001)
        c.set_batch(20)
        c.set_regions(*regions_of(plan, G))
        return c, c.run_gmm_estimation, 20, 1000000

    def mc(G):
        c = pocs_amd.Context(0)
        c.configure(long_plan, env, K=1, N=100000, seed=0x5EED0001)
        c.set_batch(64)
        c.set_option(pocs_amd.OPT_MC_FUSED, 0)
        c.set_regions(*regions_of(long_plan, G))
        return c, c.run_simulation, 64, 100000

    legs = []
    if args.only in (None, "gmm"):
        legs += [("gmm cfg2 x20, G = %d" % G, gmm(G)) for G in (0, 1, 4)]
    if args.only in (None, "mc"):
        legs += [("mc cfg5 x64 per-step, G = %d" % G, mc(G)) for G in (0, 1, 4)]
    times, probs = {name: [] for name, _ in legs}, {}
    for it in range(args.warm + args.reps):
        for name, (c, run, _, _) in legs:
            t0 = time.perf_counter()
            p = run()
            dt = time.perf_counter() - t0
            if it >= args.warm:
                times[name].append(dt * 1e3)
            probs[name] = p
    out = ["wall time of one call; %d alternating repeats after %d warm-up calls; %s" % (args.reps, args.warm, legs[0][1][0].lib.pocs_version().decode())]
    for name, _ in legs:
        t = sorted(times[name])
        base = statistics.median(times[name.split(", G")[0] + ", G = 0"])
        out.append("%-36s median %8.3f ms   min %8.3f   max %8.3f   x %.4f of G = 0   (p of last call %.6f)" % (name, statistics.median(t), t[0], t[-1], statistics.median(t) / base, probs[name]))
    for name, (c, _, R, N) in legs:
        if len(c.regions()[1]):
            tot, rows = None, 0
            for r in range(R):
                c.select_batch_run(r)
                A = c.region_counts()
                tot = A.sum(axis=0) if tot is None else tot + A.sum(axis=0)
                rows += A.shape[0]
            share = [float(v) / (rows * N) for v in tot]      # (rows: the waypoints of all runs)
            out.append("%-36s last call, share of %s counted per region: %s" % (name, "samples" if name.startswith("gmm") else "particles",
                                                                             "  ".join("%.5f" % s for s in share)))
    text = "\n".join(out)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    for _, (c, _, _, _) in legs:
        c.close()


if __name__ == "__main__":
    main()
