#!/usr/bin/env python3
"""What POCS_OPT_OBSTACLE_COUNTS costs when it is on (DESIGN.md sections 5 and 10; profiles/obstacle_counts_vs_parent.txt).

Legs, one context each, ALTERNATING call by call, the option off against on:
  gmm   bench.py's cfg2 at 20 runs per call: the bundled 56-waypoint plan and its boxes, K = 3, 10^6 samples per run, samples
        stored (the default), the call as two sub-batches (the default at this size)
  mc    bench.py's cfg5 at 64 runs per call: the plan resampled to 500 waypoints, 10^5 particles per run, in both launch forms;
        the "off" legs run under POCS_OPT_MC_WAYPOINT_COUNTS = 1 as well as plainly, since the option brings those counts along
Timed: the wall time of one pocs_run_gmm_estimation / pocs_run_simulation call (host chains, upload, graph replay, read-back;
the table itself is read by the getter, outside the call).  Median, min and max of the repeats, in ms.  For the gmm leg
under the option it also prints how many (run, waypoint) rows of the last call's tables hold a hit at all and the touched
boxes per sample: what the counting form's extra work is proportional to.

  python tools/obstacle_counts_probe.py [--reps 15] [--warm 4] [--only gmm|mc] [--off-only] [--out FILE]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import pocs_amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--only", default=None, choices=["gmm", "mc"])
    ap.add_argument("--off-only", action="store_true", help="one option-off gmm leg and one mc leg, nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    long_plan = pocs_amd.resample_plan(plan, 500)

    def gmm(on):
        c = pocs_amd.Context(0)
        c.configure(plan, env, K=3, N=1000000, seed=0x5EED0001)
        c.set_batch(20)
        c.set_option(pocs_amd.OPT_OBSTACLE_COUNTS, on)
        return c, c.run_gmm_estimation

    def mc(on, fused, wp=0):
        c = pocs_amd.Context(0)
        c.configure(long_plan, env, K=1, N=100000, seed=0x5EED0001)
        c.set_batch(64)
        c.set_option(pocs_amd.OPT_MC_FUSED, fused)
        c.set_option(pocs_amd.OPT_MC_WAYPOINT_COUNTS, wp)
        c.set_option(pocs_amd.OPT_OBSTACLE_COUNTS, on)
        return c, c.run_simulation

    legs = []
    if args.off_only:
        legs = [("gmm cfg2 x20, option off", gmm(0)), ("mc cfg5 x64 per-step, option off", mc(0, 0)), ("mc cfg5 x64 fused, option off", mc(0, 1))]
    else:
        if args.only in (None, "gmm"):
            legs += [("gmm cfg2 x20, option off", gmm(0)), ("gmm cfg2 x20, option ON", gmm(1))]
        if args.only in (None, "mc"):
            for fused, form in ((0, "per-step"), (1, "fused")):
                legs += [("mc cfg5 x64 %s, option off" % form, mc(0, fused)),
                         ("mc cfg5 x64 %s, option off, waypoint counts on" % form, mc(0, fused, 1)),
                         ("mc cfg5 x64 %s, option ON" % form, mc(1, fused))]
    times, probs = {name: [] for name, _ in legs}, {}
    for it in range(args.warm + args.reps):
        for name, (c, run) in legs:
            t0 = time.perf_counter()
            p = run()
            dt = time.perf_counter() - t0
            if it >= args.warm:
                times[name].append(dt * 1e3)
            probs[name] = p
    out = ["wall time of one call; %d alternating repeats after %d warm-up calls; %s" % (args.reps, args.warm, legs[0][1][0].lib.pocs_version().decode())]
    for name, _ in legs:
        t = sorted(times[name])
        out.append("%-56s median %8.3f ms   min %8.3f   max %8.3f   (p of last call %.6f)" % (name, statistics.median(t), t[0], t[-1], probs[name]))
    for name, (c, _) in legs:
        if name.startswith("gmm") and name.endswith("ON"):          # how rare hits are on this workload
            rows = hit_rows = touches = 0
            for r in range(20):
                c.select_batch_run(r)
                A = c.obstacle_counts()
                rows += A.shape[0]
                hit_rows += int(np.count_nonzero(A.sum(axis=1)))
                touches += int(A.sum())
            out.append("gmm, last call: %d of %d (run, waypoint) rows hold a hit; %.4f touched boxes per sample" % (hit_rows, rows, touches / (rows * 1e6)))
    text = "\n".join(out)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    for _, (c, _) in legs:
        c.close()


if __name__ == "__main__":
    main()
