#!/usr/bin/env python3
"""What a compound footprint (pocs_set_footprint_parts) costs a call.

Legs, one context each, ALTERNATING call by call: the single footprint (F = 1: the default kernels) against F = 2 and F = 4, whose
part 0 is that footprint -- the other parts are bars along its axes that reach a little past it:
  gmm   bench.py's cfg2 at 20 runs per call: the bundled 56-waypoint plan and its boxes, K = 3, 10^6 samples per run, samples
        stored (the default), the call as two sub-batches (the default at this size)
  mc    bench.py's cfg5 at 64 runs per call in the per-step form: the plan resampled to 500 waypoints, 10^5 particles per run
Timed: the wall time of one pocs_run_gmm_estimation / pocs_run_simulation call (host chains, upload, graph replay, read-back: the
call ends in a device synchronise).  Median, min and max of the repeats in ms, the median per waypoint, and the ratio of the
medians to the single footprint's.

  python tools/footprint_parts_probe.py [--reps 15] [--warm 4] [--only gmm|mc] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import pocs_amd  # noqa: E402

# (bars that reach 1.6 cm past the bundled square footprint: the room's collision probabilities stay what a user's would be -- parts that
# stick far out collide everywhere in this room, and a call whose samples all collide is not the workload)
EXTRA = [(0.05, 0.0, 0.3, 0.1), (0.0, 0.05, 0.1, 0.3), (-0.05, 0.0, 0.3, 0.1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["gmm", "mc"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    long_plan = pocs_amd.resample_plan(plan, 500)

    def parts(F):
        return [tuple(env["footprint"])] + EXTRA[:F - 1]

    def gmm(F):
        c = pocs_amd.Context(0)
        c.configure(plan, env, K=3, N=1000000, seed=0x5EED0001)
        c.set_batch(20)
        if F > 1:
            c.set_footprint_parts(parts(F))
        return c, c.run_gmm_estimation, len(plan["traj"])

    def mc(F):
        c = pocs_amd.Context(0)
        c.configure(long_plan, env, K=1, N=100000, seed=0x5EED0001)
        c.set_batch(64)
        c.set_option(pocs_amd.OPT_MC_FUSED, 0)
        if F > 1:
            c.set_footprint_parts(parts(F))
        return c, c.run_simulation, len(long_plan["traj"])

    legs = []
    if args.only in (None, "gmm"):
        legs += [("gmm cfg2 x20, F = %d" % F, gmm(F)) for F in (1, 2, 4)]
    if args.only in (None, "mc"):
        legs += [("mc cfg5 x64 per-step, F = %d" % F, mc(F)) for F in (1, 2, 4)]
    times, probs = {name: [] for name, _ in legs}, {}
    for it in range(args.warm + args.reps):
        for name, (c, run, _) in legs:
            t0 = time.perf_counter()
            p = run()
            dt = time.perf_counter() - t0
            if it >= args.warm:
                times[name].append(dt * 1e3)
            probs[name] = p
    out = ["wall time of one call; %d alternating repeats after %d warm-up calls; %s" % (args.reps, args.warm, legs[0][1][0].lib.pocs_version().decode())]
    base = {}
    for name, (_, _, W) in legs:
        t = sorted(times[name])
        med = statistics.median(t)
        kind = name.split(",")[0]
        base.setdefault(kind, med)
        out.append("%-32s median %9.3f ms   min %9.3f   max %9.3f   per waypoint %8.4f ms   x %.3f of F = 1   (p of last call %.6f)"
                   % (name, med, t[0], t[-1], med / W, med / base[kind], probs[name]))
    text = "\n".join(out)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    for _, (c, _, _) in legs:
        c.close()


if __name__ == "__main__":
    main()
