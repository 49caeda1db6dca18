#!/usr/bin/env python3
"""What clearance levels (pocs_set_clearance_levels) cost when they are on (DESIGN.md sections 5 and 10).

Legs, one context each, ALTERNATING call by call, L = 0 against L = 1 (0.05) and L = 3 (0.01, 0.03, 0.08):
  gmm   bench.py's cfg2 at 20 runs per call: the bundled 56-waypoint plan and its boxes, K = 3, 10^6 samples per run, samples
        stored (the default), the call as two sub-batches (the default at this size)
  mc    bench.py's cfg5 at 64 runs per call in the per-step form: the plan resampled to 500 waypoints, 10^5 particles per run
Timed: the wall time of one pocs_run_gmm_estimation / pocs_run_simulation call (host chains, upload, graph replay, read-back, the
table's copy included).  Median, min and max of the repeats, in ms; for the legs under levels, the share of samples / particles
the last call's table counts per level.

  python tools/clearance_probe.py [--reps 15] [--warm 4] [--only gmm|mc] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import pocs_amd  # noqa: E402

LEVELS = {0: (), 1: (0.05,), 3: (0.01, 0.03, 0.08)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["gmm", "mc"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    long_plan = pocs_amd.resample_plan(plan, 500)

    def gmm(L):
        c = pocs_amd.Context(0)
        c.configure(plan, env, K=3, N=1000000, seed=0x5EED0001)
        c.set_batch(20)
        c.set_clearance_levels(LEVELS[L])
        return c, c.run_gmm_estimation, 20, 1000000

    def mc(L):
        c = pocs_amd.Context(0)
        c.configure(long_plan, env, K=1, N=100000, seed=0x5EED0001)
        c.set_batch(64)
        c.set_option(pocs_amd.OPT_MC_FUSED, 0)
        c.set_clearance_levels(LEVELS[L])
        return c, c.run_simulation, 64, 100000

    legs = []
    if args.only in (None, "gmm"):
        legs += [("gmm cfg2 x20, L = %d" % L, gmm(L)) for L in (0, 1, 3)]
    if args.only in (None, "mc"):
        legs += [("mc cfg5 x64 per-step, L = %d" % L, mc(L)) for L in (0, 1, 3)]
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
        out.append("%-36s median %8.3f ms   min %8.3f   max %8.3f   (p of last call %.6f)" % (name, statistics.median(t), t[0], t[-1], probs[name]))
    for name, (c, _, R, N) in legs:
        if len(c.clearance_levels()):
            tot, rows = None, 0
            for r in range(R):
                c.select_batch_run(r)
                A = c.clearance_counts()
                tot = A.sum(axis=0) if tot is None else tot + A.sum(axis=0)
                rows += A.shape[0]
            share = [float(v) / (rows * N if name.startswith("gmm") else R * N) for v in tot]
            out.append("%-36s last call, share of %s counted per level: %s" % (name, "samples" if name.startswith("gmm") else "particles",
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
