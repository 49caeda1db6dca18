#!/usr/bin/env python3
"""What the fused MC roll-out costs under an obstacle schedule (pocs_set_obstacle_schedule, k_mc_fused_sched), against the
launch forms of ANOTHER build of the library under a static world -- the parent commit's, to decide whether the scheduled
fused kernel ships (DESIGN.md sections 5 and 7; profiles/obstacle_schedule_vs_parent.txt).

Shape: the bundled 56-waypoint plan and its boxes, one run per call, --particles per run.  Schedules of S = 56 steps:
  nudged     world s = the bundled boxes with every centre x and yaw moved by 1e-3 * s: no two tables are equal.  These worlds
             collide more often than the bundled one, so a nudged leg does more collision work than a static leg
  repeated   world s = the bundled boxes, 56 times: the static world's work exactly, restaged per step
Legs: this build -- nudged fused, nudged per-step, repeated fused, static per-step, static fused; the other build (--parent-lib)
-- static per-step, static fused.  Both libraries are loaded into this ONE process (the second through POCS_LIB, as
capi.load_library reads it), one context per leg, and the legs ALTERNATE call by call.  Timed: the wall time of one
pocs_run_simulation call (host chain, upload, graph replay, read-back).  Median, min and max of the repeats, in ms.

The other build: check the parent commit out somewhere and compile its csrc/*.hip with build.py's FLAGS into a libpocs.so.

  python tools/obstacle_schedule_probe.py --parent-lib /path/to/parent/libpocs.so [--particles 1000000] [--reps 15] [--warm 4] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time
from importlib import import_module
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import pocs_amd  # noqa: E402

capi = import_module("probability-of-collision-for-safe-planning_amd.capi")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libpocs.so of the build to compare against")
    ap.add_argument("--particles", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warm", type=int, default=4)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    plan, env = pocs_amd.load_plan(), pocs_amd.load_env()
    boxes = np.asarray(env["boxes"], dtype=np.float64).reshape(-1, 5)
    W, M = len(plan["traj"]), len(boxes)
    S = W
    repeated = pocs_amd.moving_boxes(boxes, np.zeros((M, 3)), S)
    nudged = pocs_amd.moving_boxes(boxes, np.tile([1e-3, 0.0, 1e-3], (M, 1)), S)

    def make(fused, sched=None):
        c = pocs_amd.Context(0)
        c.configure(plan, env, K=3, N=args.particles, seed=0x5EED0001)
        c.set_option(pocs_amd.OPT_MC_FUSED, fused)
        if sched is not None:
            c.set_obstacle_schedule(sched)
        return c

    legs = [("this build, nudged schedule S=%d, fused (k_mc_fused_sched)" % S, make(1, nudged)),
            ("this build, nudged schedule S=%d, per-step" % S, make(0, nudged)),
            ("this build, repeated schedule S=%d, fused (k_mc_fused_sched)" % S, make(1, repeated)),
            ("this build, static world, per-step", make(0)),
            ("this build, static world, fused", make(1))]
    capi._lib = None                                   # the second library: capi loads whatever POCS_LIB names
    os.environ["POCS_LIB"] = str(Path(args.parent_lib).resolve())
    legs[1:1] = [("other build, static world, per-step (POCS_OPT_MC_FUSED=0)", make(0)),
                 ("other build, static world, fused (POCS_OPT_MC_FUSED=1)", make(1))]
    assert legs[1][1].lib is not legs[0][1].lib
    times, probs = {name: [] for name, _ in legs}, {}
    for it in range(args.warm + args.reps):
        for name, c in legs:
            t0 = time.perf_counter()
            p = c.run_simulation()
            dt = time.perf_counter() - t0
            if it >= args.warm:
                times[name].append(dt * 1e3)
            probs[name] = p
    out = ["MC roll-out, N = %d particles, W = %d waypoints, M = %d boxes, one run per call; wall time of one pocs_run_simulation call;"
           % (args.particles, W, M),
           "%d alternating repeats after %d warm-up calls; this build %s; other build %s"
           % (args.reps, args.warm, legs[0][1].lib.pocs_version().decode(), legs[1][1].lib.pocs_version().decode())]
    for name, _ in legs:
        t = sorted(times[name])
        out.append("%-62s median %8.3f ms   min %8.3f   max %8.3f   (p of last call %.6f)"
                   % (name, statistics.median(t), t[0], t[-1], probs[name]))
    text = "\n".join(out)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
